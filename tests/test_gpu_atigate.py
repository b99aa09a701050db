"""The GMTI ATI gate on the device (include/sarx_atigate.h, csrc/atigate.hip, sarx/atigate.py) against the restatement of
tests/_atigate_numpy.py.

Parity of the sums.  Every term of a sum is the exact fp64 product of two fp32 samples (24 x 24 bits fit 53), so the device and
the restatement add the SAME real numbers t_1 .. t_m and differ only in how they round.  The restatement's math.fsum is the
correctly rounded exact sum S.  A floating-point summation of m terms in ANY order (any tree) returns S_hat with
|S_hat - S| <= (m - 1) u sum|t_k| + O(u^2) for u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2),
and fsum adds at most u |S| <= u sum|t_k|.  With eps = 2^-52 = 2 u:
  c11, c22 : m = 2 N terms (re^2 and im^2 per cell), all >= 0, so sum|t_k| = S:  |c11 - ref| <= m u S = N eps ref.
  c12      : each component has m = 2 N terms of either sign: |component - ref| <= m u sum|t_k| = N eps sum|t_k|, inside the
             2 N eps sum|t_k| held here.
  I        : the same with n_look for N.
Derived values.  With coh in [0.3, 0.99] and |I| >= 0.1 sum_L |a||b| (asserted on the restatement's values for every tested
report) first-order propagation of those bounds gives: d coh <= coh (dc12 / |c12| + dc11 / 2 c11 + dc22 / 2 c22) <=
N eps (2 sqrt(2) / 0.3 + 1) ~ 1e-12 at N = 4200; d psi <= d angle(I) + d angle(c12) <= sqrt(2) (2 n_look eps / 0.1 + 2 N eps / 0.3)
~ 1e-11; d sigma / sigma = d coh / (coh (1 - coh^2)) <= 1e-12 / (0.3 x 0.02) ~ 2e-10 at worst, 1e-11 over most of the range; the
library functions (sqrt, hypot, atan2) add a few eps.  The bounds held are 1e-9 absolute for coh and psi and 1e-9 relative for
sigma.
Decisions.  status must equal step 5 applied in NumPy to the device's own psi and sigma, exactly; and the restatement's status
wherever the restatement's margin ||psi| - thr| exceeds 1e-7 - the seeds below were chosen on the CPU, with the restatement alone,
so that no report of any case lies inside that band, and every case asserts it: the share of reports left out is 0."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _atigate_numpy as ref  # noqa: E402
from test_atigate import scene_reports  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
N_AZ, N_RG = 96, 80
WINDOWS = {"small": ((0, 0), (1, 1), (0, 0)), "default": ((2, 2), (8, 8), (1, 1)), "wide": ((4, 2), (28, 30), (4, 2))}
SEEDS = {"small": 1, "default": 1, "wide": 1, "counts": 1, "tiny": 1}      # chosen on the CPU: see the docstring
BAND = 1e-7


class Out:
    """One frame's outputs as downloaded, whole buffers (poisoned with 0xFF before the launch)."""

    def __init__(self, slot, stats_raw, n_in):
        self.slot, self.stats_raw = slot, stats_raw
        self.header = slot[:16].view("<u4")
        k = min(int(self.header[0]), (len(slot) - 16) // 48)
        self.n_kept = k
        self.reports = slot[16:16 + 48 * k].view(ref.REPORT_DTYPE)
        self.stats = None if stats_raw is None else stats_raw[:96 * n_in].view(ref.STAT_DTYPE)


def gate_params(kw):
    import sarx
    names = dict(guard="guard", train="train", looks="looks", k_sigma="k_sigma", phase_min="phase_min", min_coh="min_coh",
                 min_train="min_train", keep_untested="keep_untested")
    return sarx.AtiGateParams(**{names[k]: v for k, v in kw.items() if k in names})


def device_step(raw, a, b, kw, md, want_stats=True, n_in=None):
    """sarx_atigate_step_dev on the slot bytes `raw` and the images a, b ([n_az x n_rg] complex64)."""
    import sarx
    from sarx import atigate as K
    ctx = sarx.default_context()
    cp = gate_params(kw).c_params(md)
    n_az, n_rg = a.shape
    bufs = [ctx.to_device(raw), ctx.to_device(np.ascontiguousarray(a, np.complex64)), ctx.to_device(np.ascontiguousarray(b, np.complex64)),
            ctx.alloc(16 + 48 * md), ctx.alloc(96 * md)]
    try:
        d_in, d_a, d_b, d_out, d_stats = bufs
        for x in (d_out, d_stats):
            sarx._ffi.check(ctx.lib.sarx_memset(ctx.h, x.ptr, 0xFF, x.nbytes), ctx.h)
        K.enqueue_step(ctx, cp, d_a.ptr, d_b.ptr, n_az, n_rg, d_in.ptr, d_out.ptr, d_stats.ptr if want_stats else None)
        n = int(raw[:4].view("<u4")[0]) if n_in is None else n_in
        return Out(d_out.download(np.uint8, (d_out.nbytes,)).copy(), d_stats.download(np.uint8, (d_stats.nbytes,)).copy(), min(n, md))
    finally:
        for x in bufs:
            x.release()


def check_sums(got, want):
    """The six sums of every report inside the bounds of the docstring; the counts exactly.  Prints the largest share of each bound
    that is used."""
    g, w, ab = got.stats, want.stats, want.abs
    assert np.array_equal(g["n_train"], w["n_train"]) and np.array_equal(g["n_look"], w["n_look"])
    n_of = dict(c11=w["n_train"], c22=w["n_train"], c12_re=w["n_train"], c12_im=w["n_train"], i_re=w["n_look"], i_im=w["n_look"])
    used = {}
    for name in ref.SUMS:
        n = n_of[name].astype(np.float64)
        bound = n * EPS * w[name] if name in ("c11", "c22") else 2.0 * n * EPS * ab[name]
        err = np.abs(g[name] - w[name])
        used[name] = float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))
        assert (err <= bound).all(), (name, int(np.argmax(err - bound)), float(np.max(err - bound)))
    print("share of the bound used:", {k: f"{v:.3f}" for k, v in used.items()})


def check_derived(got, want, rep, a, b, looks):
    """coh, psi to 1e-9 absolute, sigma to 1e-9 relative, on inputs that meet the conditions of the docstring (asserted)."""
    g, w = got.stats, want.stats
    tested = w["status"] != ref.UNTESTED
    assert tested.any()
    assert np.array_equal(g["reason"], w["reason"])
    coh = w["coh"][tested]
    assert (coh >= 0.3).all() and (coh <= 0.99).all(), (coh.min(), coh.max())
    mag = np.abs(a.astype(np.complex128)) * np.abs(b.astype(np.complex128))
    for r in np.flatnonzero(tested):                                    # |I| >= 0.1 sum over the look box of |a||b|
        i, j = int(rep["i"][r]), int(rep["j"][r])
        box = mag[max(i - looks[0], 0):i + looks[0] + 1, max(j - looks[1], 0):j + looks[1] + 1]
        assert np.hypot(w["i_re"][r], w["i_im"][r]) >= 0.1 * box.sum(), r
    assert np.max(np.abs(g["coh"] - w["coh"])) <= 1e-9
    dpsi = np.abs(g["psi"] - w["psi"])
    dpsi = np.minimum(dpsi, 2.0 * np.pi - dpsi)                        # a phase at +-pi may come out on either side
    assert np.max(dpsi) <= 1e-9
    assert np.max(np.abs(g["sigma"][tested] - w["sigma"][tested]) / w["sigma"][tested]) <= 1e-9
    assert not g["coh"][w["reason"] == 1].any() and not g["psi"][~tested].any() and not g["sigma"][~tested].any()
    print(f"derived: max |d coh| {np.max(np.abs(g['coh'] - w['coh'])):.2e}, max |d psi| {np.max(dpsi):.2e}, "
          f"max rel d sigma {np.max(np.abs(g['sigma'][tested] - w['sigma'][tested]) / w['sigma'][tested]):.2e}")


def check_decisions(got, want, kw):
    """status from the device's own psi and sigma, exactly; the restatement's status outside the band - and nobody inside it."""
    g, w = got.stats, want.stats
    tested = w["status"] != ref.UNTESTED
    own = ref.decide(g["psi"], g["sigma"], kw.get("k_sigma", 3.0), kw.get("phase_min", 0.0))
    assert np.array_equal(g["status"][tested], own[tested]) and not g["status"][~tested].any()
    margin = np.abs(np.abs(w["psi"][tested]) - want.thr[tested])
    assert (margin > BAND).all(), "a report inside the band: choose another seed (on the CPU)"
    assert np.array_equal(g["status"], w["status"])
    assert not g["reserved"].any()


def check_slot(got, want, raw_in, keep_untested):
    """The output slot = the kept input reports byte for byte, out_index consistent, nothing past the promised bytes touched."""
    rep_in = raw_in[16:16 + 48 * len(want.stats)].view(ref.REPORT_DTYPE)
    g = got.stats
    kept = (g["status"] == ref.PASSED) | ((g["status"] == ref.UNTESTED) & keep_untested)
    assert got.header.tolist() == [int(kept.sum()), 0, 0, 0] == want.header.tolist()
    assert got.reports.tobytes() == rep_in[kept].tobytes() == want.reports.tobytes()
    assert np.array_equal(g["out_index"], np.where(kept, np.cumsum(kept) - 1, -1)) and np.array_equal(g["out_index"], want.stats["out_index"])
    assert (got.slot[16 + 48 * got.n_kept:] == 0xFF).all() and (got.stats_raw[96 * len(g):] == 0xFF).all()


def run_case(a, b, rep, kw, md, sums_of=None, derived=True):
    want = ref.gate(rep, a, b, max_detections=md, sums_of=sums_of, **kw)
    raw = ref.slot_bytes(rep, md)
    got = device_step(raw, a, b, kw, md)
    check_sums(got, want)
    if derived:
        check_derived(got, want, rep, a, b, kw.get("looks", (1, 1)))
    check_decisions(got, want, kw)
    check_slot(got, want, raw, kw.get("keep_untested", True))
    return want, got, raw


# ---- windows: corners, edges, interior ----------------------------------------------------------------------------------------------------
def placed_cells(seed, n_interior=20):
    """All four corners, three cells on every edge, one cell next to a corner, and interior cells of a 96 x 80 image."""
    rng = np.random.default_rng(seed)
    cells = {(0, 0), (0, N_RG - 1), (N_AZ - 1, 0), (N_AZ - 1, N_RG - 1), (1, 1), (N_AZ - 2, N_RG - 3)}
    for k in range(3):
        cells |= {(0, int(rng.integers(1, N_RG - 1))), (N_AZ - 1, int(rng.integers(1, N_RG - 1))),
                  (int(rng.integers(1, N_AZ - 1)), 0), (int(rng.integers(1, N_AZ - 1)), N_RG - 1)}
    while len(cells) < 18 + n_interior:
        cells.add((int(rng.integers(2, N_AZ - 2)), int(rng.integers(2, N_RG - 2))))
    return sorted(cells)


@functools.lru_cache(maxsize=None)
def window_case(name):
    guard, train, looks = WINDOWS[name]
    seed = SEEDS[name]
    a, b = ref.parity_scene(100 + seed, N_AZ, N_RG, coherence=0.6 if name == "small" else 0.8)
    rep = ref.make_reports(placed_cells(seed), seed=seed)
    # min_train = 1: the corners are tested too; k_sigma = 1: clutter alone passes about a third of the time, so both decisions occur
    kw = dict(guard=guard, train=train, looks=looks, k_sigma=1.0, min_train=1)
    return a, b, rep, kw, ref.sums(rep, a, b, guard, train, looks)


@pytest.mark.parametrize("name", list(WINDOWS))
def test_windows_at_corners_edges_and_interior(name):
    a, b, rep, kw, sums_of = window_case(name)
    want, got, _ = run_case(a, b, rep, kw, 64, sums_of)
    nf = ref.n_full(kw["guard"], kw["train"])
    n_train = want.stats["n_train"]
    assert n_train.min() < nf / 2 and n_train.max() == nf              # clipped at the corners, whole in the interior (65 <= 80)
    assert (want.stats["status"] != ref.UNTESTED).all() and {ref.PASSED, ref.REJECTED} <= set(want.stats["status"].tolist())
    if name == "wide":                                  # outer half-width 32: 65 columns, one more than a wave has lanes
        assert kw["guard"][1] + kw["train"][1] == 32 and kw["guard"][0] + kw["train"][0] == 32


# ---- report counts that are multiples of neither a wave nor the workgroup -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def count_case(n):
    seed = SEEDS["counts"]
    a, b = ref.parity_scene(200 + seed, N_AZ, N_RG)
    flat = np.random.default_rng(300 + seed + n).choice(N_AZ * N_RG, n, replace=False)
    rep = ref.make_reports(np.stack([flat // N_RG, flat % N_RG], axis=1), seed=n)
    return a, b, rep, ref.sums(rep, a, b)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("n", [0, 1, 65, 1025])
def test_report_counts_and_keep_untested(n, keep):
    """Random cells of the whole image with the default window and the default min_train: cells near the edge are untested
    (reason 1), kept or dropped by the flag."""
    a, b, rep, sums_of = count_case(n)
    kw = dict(k_sigma=1.0, keep_untested=keep)
    want, got, raw = run_case(a, b, rep, kw, 1100, sums_of, derived=n > 1)
    st = want.stats
    if n >= 65:
        assert (st["reason"] == 1).any() and (st["status"] == ref.PASSED).any() and (st["status"] == ref.REJECTED).any()
        assert got.n_kept == int(((st["status"] == ref.PASSED) | (keep & (st["status"] == ref.UNTESTED))).sum()) < n
    if n == 1025:                                       # two runs give identical bytes
        again = device_step(raw, a, b, kw, 1100)
        assert np.array_equal(again.slot, got.slot) and np.array_equal(again.stats_raw, got.stats_raw)
        bare = device_step(raw, a, b, kw, 1100, want_stats=False)         # statistics left out: the same slot, the buffer untouched
        assert np.array_equal(bare.slot, got.slot) and (bare.stats_raw == 0xFF).all()


def test_zero_thresholds_copy_the_slot():
    a, b, rep, sums_of = count_case(1025)
    kw = dict(k_sigma=0.0, phase_min=0.0, keep_untested=True)
    want, got, raw = run_case(a, b, rep, kw, 1100, sums_of)
    assert got.n_kept == 1025 and np.array_equal(got.slot[:16 + 48 * 1025], raw[:16 + 48 * 1025])
    assert np.array_equal(got.stats["out_index"], np.arange(1025))


def test_image_smaller_than_the_window():
    """5 x 7 image, train (8, 8): the outer box covers the image from every cell, N = 35 - |guard box| = 10 .. 26, and min_train = 20
    decides who is tested."""
    a, b = ref.parity_scene(400 + SEEDS["tiny"], 5, 7)
    rep = ref.make_reports([[i, j] for i in range(5) for j in range(7)], seed=5)
    for keep in (True, False):
        kw = dict(min_train=20, keep_untested=keep)
        want, got, _ = run_case(a, b, rep, kw, 35, derived=False)
        st = want.stats
        assert st["n_train"].min() == 10 and st["n_train"].max() == 26
        assert np.array_equal(st["reason"] == 1, st["n_train"] < 20) and (st["reason"] == 1).any() and (st["reason"] == 0).any()


def test_all_zero_images_are_untested():
    z = np.zeros((N_AZ, N_RG), np.complex64)
    _, _, rep, _ = count_case(65)
    for keep in (True, False):
        want, got, raw = run_case(z, z, rep, dict(min_train=1, keep_untested=keep), 100, derived=False)
        assert (got.stats["reason"] == 2).all() and (got.stats["status"] == ref.UNTESTED).all()
        for name in ref.SUMS + ("coh", "psi", "sigma"):
            assert not got.stats[name].any(), name
        assert got.n_kept == (65 if keep else 0)
        if keep:
            assert np.array_equal(got.slot[:16 + 48 * 65], raw[:16 + 48 * 65])


@pytest.mark.parametrize("kw", [dict(overflow=1), dict(count=65)])
def test_overflow_in_overflow_out(kw):
    import sarx
    a, b, rep, _ = count_case(65)
    rep = rep[:64]
    raw = ref.slot_bytes(rep, 64, **kw)
    got = device_step(raw, a, b, {}, 64, n_in=0)
    assert got.header.tolist() == [kw.get("count", 64), 1, 0, 0] == ref.gate(rep, a, b, max_detections=64, **kw).header.tolist()
    assert (got.slot[16:] == 0xFF).all() and (got.stats_raw == 0xFF).all()
    with pytest.raises(sarx.GmtiOverflowError) as e:
        sarx.gmti_ati_gate(raw, a.T, b.T, max_detections=64)
    assert e.value.count == kw.get("count", 64)


def test_arguments_the_header_forbids():
    """Past the context check, on the device: overlap, alignment, sizes - SARX_ERR_INVALID and nothing launched."""
    import ctypes as C
    import sarx
    ctx = sarx.default_context()
    md = 8
    cp = sarx.AtiGateParams().c_params(md)
    slot, rec, img = 16 + 48 * md, 96 * md, 16 * 16 * 8
    buf = ctx.alloc(2 * img + 4 * slot + 2 * rec)
    try:
        a, b = buf.ptr, buf.ptr + img
        p = buf.ptr + 2 * img
        s = p + 4 * slot
        step = lambda *args: ctx.lib.sarx_atigate_step_dev(ctx.h, C.byref(cp), *args)
        bad = [step(a, b, 16, 16, p, p, None), step(a, b, 16, 16, p, p + slot - 8, None), step(a, b, 16, 16, p, a + 8, None),
               step(a, b, 16, 16, p, p + slot, p + 8), step(a, b, 16, 16, p, p + slot, p + slot + 16), step(a, b, 16, 16, p, p + slot, b),
               step(a + 4, b, 16, 16, p, p + slot, s), step(a, b, 16, 16, p + 4, p + slot, s), step(a, b, 16, 16, p, p + slot, s + 4),
               step(None, b, 16, 16, p, p + slot, s), step(a, b, 16, 16, None, p + slot, s), step(a, b, 0, 16, p, p + slot, s),
               step(a, b, 16, -1, p, p + slot, s)]
        assert all(rc != 0 for rc in bad), bad
        assert len(ctx.lib.sarx_last_error(ctx.h)) > 10
        sarx._ffi.check(ctx.lib.sarx_memset(ctx.h, buf.ptr, 0, buf.nbytes), ctx.h)
        assert step(a, b, 16, 16, p, p + slot, s) == 0                                  # and the plain call still goes (count 0)
        ctx.sync()
    finally:
        buf.release()


# ---- the Python interface, and end to end -------------------------------------------------------------------------------------------------
AXES = dict(range_axis=1000.0 + 2.0 * np.arange(128), cross_range=-32.0 + 0.5 * np.arange(128))
RADAR = dict(wavelength_m=0.03, platform_speed_mps=100.0, lag_s=1e-3)


def test_gmti_ati_gate_takes_every_kind_of_input():
    import sarx
    from sarx import gmti
    a, b, truth, rep = scene_reports()
    det = sarx.GmtiParams(max_detections=64)
    want = ref.gate(rep, a, b, max_detections=64)
    raw = ref.slot_bytes(rep, 64)
    report = gmti.decode_slot(raw, det, AXES["range_axis"], AXES["cross_range"], 0.03, 100.0, 1e-3)
    ctx = sarx.default_context()
    held = ctx.to_device(raw)
    try:
        outs = [sarx.gmti_ati_gate(x, a.T, b.T, sarx.AtiGateParams(), detect=det, **AXES, **RADAR)
                for x in (report, rep.astype(gmti.REPORT_DTYPE), raw, held)]
    finally:
        held.release()
    for gated, gate in outs:
        assert isinstance(gated, sarx.GmtiReport) and len(gated) == 5 and gated.gate is gate
        assert list(zip(gated.detections["i"].tolist(), gated.detections["j"].tolist())) == truth["movers"]
        assert np.array_equal(gate["status"], want.stats["status"]) and np.array_equal(gate["out_index"], want.stats["out_index"])
        assert gate.tobytes() == outs[0][1].tobytes()
    # the report's own fields travel through unchanged (from the raw forms; a GmtiReport carries no reserved bytes to compare)
    bare, gate = sarx.gmti_ati_gate(rep.astype(gmti.REPORT_DTYPE), a.T, b.T)            # no axes: the kept reports as an array
    assert bare.dtype == gmti.REPORT_DTYPE and bare.tobytes() == want.reports.tobytes() and len(gate) == len(rep)
    none, gate = sarx.gmti_ati_gate(ref.make_reports([]), a.T, b.T)
    assert len(none) == 0 and len(gate) == 0


def test_gmti_detect_with_the_gate_returns_exactly_the_movers():
    """End to end on the 128 x 128 scene of tests/test_atigate.py: without the gate the detector also reports the stationary
    scatterers that leak through DPCA; with it exactly the movers' reports come back, byte for byte those of the ungated list, and go
    through cluster= and sarx.gmti_refocus unchanged."""
    import sarx
    from sarx import cluster as clu
    a, b, truth, _ = scene_reports()
    kw = dict(pfa=1e-9, cal_phase=truth["cal_phase"], max_detections=64, **RADAR)
    plain = sarx.gmti_detect(a.T, b.T, AXES["range_axis"], AXES["cross_range"], **kw)
    cells = lambda rep: list(zip(rep.detections["i"].tolist(), rep.detections["j"].tolist()))
    assert cells(plain) == sorted(truth["statics"] + truth["movers"]) and plain.gate is None
    gated = sarx.gmti_detect(a.T, b.T, AXES["range_axis"], AXES["cross_range"], ati_gate=sarx.AtiGateParams(), **kw)
    assert cells(gated) == truth["movers"]
    is_mover = np.array([c in truth["movers"] for c in cells(plain)])
    assert gated.detections.tobytes() == plain.detections[is_mover].tobytes()
    assert len(gated.gate) == len(plain) and np.array_equal(gated.gate["status"] == ref.PASSED, is_mover)
    assert (gated.gate["status"][~is_mover] == ref.REJECTED).all()
    for c, psi in zip(cells(gated), gated.gate["psi"][is_mover]):
        assert abs(psi - truth["mover_phases"][c]) < 0.1
    # cluster= works on the gated slot: with link (0, 0) its plot list IS the gated list
    both = sarx.gmti_detect(a.T, b.T, AXES["range_axis"], AXES["cross_range"], ati_gate=sarx.AtiGateParams(),
                            cluster=sarx.ClusterParams(link=(0, 0)), **kw)
    assert both.detections.tobytes() == gated.detections.tobytes() and both.plots.n_plots == 5 and both.plots.n_reports == 5
    assert both.plots.detections.detections.tobytes() == gated.detections.tobytes()
    assert isinstance(both.plots, clu.GmtiPlots) and both.plots.plots["peak_report"].tolist() == [0, 1, 2, 3, 4]
    # ... and the refocus takes the gated report like any other
    rp = sarx.RefocusParams(chip=(64, 5), n_hyp=9)
    r_gated = sarx.gmti_refocus(gated, a.T, b.T, AXES["range_axis"], AXES["cross_range"], wavelength_m=0.03, platform_speed_mps=100.0,
                                prf_hz=1000.0, params=rp, cal_phase=truth["cal_phase"])
    r_cells = sarx.gmti_refocus(np.array(truth["movers"], np.int64), a.T, b.T, AXES["range_axis"], AXES["cross_range"], wavelength_m=0.03,
                                platform_speed_mps=100.0, prf_hz=1000.0, params=rp, cal_phase=truth["cal_phase"])
    assert len(r_gated.records) == 5 and r_gated.records.tobytes() == r_cells.records.tobytes()


# ---- the batch ------------------------------------------------------------------------------------------------------------------------
def test_batch_ships_the_gated_slot():
    """The 1024-pixel C3 batch of tests/test_gpu_cluster.py, two frames: with thresholds of zero the gate copies the detector's
    slot, so the stack is what it is without ati_gate=; with the default gate every slot holds a subset of those reports, byte for
    byte and in order; with cluster= the plot extraction works on the gated list."""
    import sarx
    from sarx.batch import TwoChannelBatch
    ctx = sarx.default_context()
    n, frames, md = 1024, 2, 16384
    det = sarx.GmtiParams(guard=(3, 16), train=(8, 8), pfa=1e-6, max_detections=md)
    gate = sarx.AtiGateParams(guard=(3, 16), train=(8, 8))
    link = (8, 32)
    stacks = {}
    for name, kw in (("plain", {}), ("copy", dict(ati_gate=sarx.AtiGateParams(guard=(3, 16), train=(8, 8), k_sigma=0.0))),
                     ("gated", dict(ati_gate=gate)), ("both", dict(ati_gate=gate, cluster=sarx.ClusterParams(link=link)))):
        b = TwoChannelBatch(ctx, n, frames, stack="detections", scene="c3", scene_scale=0.25, detect=det, **kw)
        b.run()
        ctx.sync()
        stacks[name] = b.stack().copy().view(np.uint8)
        assert b.slot_bytes == 16 + (48 + (64 if name == "both" else 0)) * md       # the statistics records are not shipped
        if name == "both":
            plots = [b.plots(f) for f in range(frames)]
        b.close()
    assert np.array_equal(stacks["copy"], stacks["plain"])
    for f in range(frames):
        n_all, n_kept = (int(stacks[k][f][:4].view("<u4")[0]) for k in ("plain", "gated"))
        rows = lambda k, c: [bytes(r) for r in stacks[k][f][16:16 + 48 * c].reshape(c, 48)]
        all_rows, kept_rows = rows("plain", n_all), rows("gated", n_kept)
        assert 0 < n_kept < n_all and not stacks["gated"][f][16 + 48 * n_kept:].any()
        it = iter(all_rows)
        assert all(r in it for r in kept_rows)                            # a subsequence: a subset, in order
        alone = sarx.gmti_cluster(stacks["gated"][f][:16 + 48 * n_kept], sarx.ClusterParams(link=link), detect=det)
        assert stacks["both"][f][:16 + 48 * alone.n_plots].tobytes() == alone.raw.tobytes()
        assert plots[f].n_plots == alone.n_plots and plots[f].n_reports == n_kept
        print(f"frame {f}: {n_all} reports, {n_kept} kept by the gate, {alone.n_plots} plots")
