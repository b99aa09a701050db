"""Restatement of the GMTI ATI gate (include/sarx_atigate.h states the semantics; csrc/atigate.hip implements them) - the checker
of tests/test_atigate.py and tests/test_gpu_atigate*.py.  No sarx import.

Every sum is formed by direct loops over the cells of its set, term by term as the header lists them (two exact products per cell
and component: a Python float product of two fp32 values is exact), and added with math.fsum, which returns the correctly rounded
sum of its terms whatever their order.  Beside every sum the sum of the terms' absolute values is kept: the bound a summation in
any other order is held to (tests/test_gpu_atigate.py)."""
import math

import numpy as np

REPORT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("power", "<f8"), ("mean", "<f8"), ("interf_re", "<f8"), ("interf_im", "<f8"),
                         ("mag1", "<f4"), ("mag2", "<f4")])
STAT_DTYPE = np.dtype([("c11", "<f8"), ("c22", "<f8"), ("c12_re", "<f8"), ("c12_im", "<f8"), ("i_re", "<f8"), ("i_im", "<f8"),
                       ("coh", "<f8"), ("psi", "<f8"), ("sigma", "<f8"), ("n_train", "<i4"), ("n_look", "<i4"), ("status", "<i4"),
                       ("reason", "<i4"), ("out_index", "<i4"), ("reserved", "<i4")])
assert REPORT_DTYPE.itemsize == 48 and STAT_DTYPE.itemsize == 96
SUMS = ("c11", "c22", "c12_re", "c12_im", "i_re", "i_im")
ABS_DTYPE = np.dtype([(name, "<f8") for name in SUMS])
MAX_HALF, MAX_LOOK, MAX_DETECTIONS = 32, 4, 16384
UNTESTED, REJECTED, PASSED = 0, 1, 2
KEEP_UNTESTED = 1


def n_full(guard, train):
    (ga, gr), (ta, tr) = guard, train
    return (2 * (ga + ta) + 1) * (2 * (gr + tr) + 1) - (2 * ga + 1) * (2 * gr + 1)


def make_reports(ij, seed=0):
    """Reports at the cells `ij` (an (n, 2) array, no cell twice), sorted by (i, j), every other field seeded (the gate copies them)."""
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    ij = ij[np.lexsort((ij[:, 1], ij[:, 0]))]
    assert len(ij) < 2 or not np.any((np.diff(ij[:, 0]) == 0) & (np.diff(ij[:, 1]) == 0)), "a cell twice"
    n = len(ij)
    rng = np.random.default_rng(seed)
    rep = np.zeros(n, REPORT_DTYPE)
    rep["i"], rep["j"] = ij[:, 0], ij[:, 1]
    rep["power"] = 20.0 + rng.exponential(30.0, n)
    rep["mean"] = 1.0 + rng.random(n)
    rep["interf_re"], rep["interf_im"] = rng.normal(size=n), rng.normal(size=n)
    rep["mag1"], rep["mag2"] = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
    return rep


def slot_bytes(reports, max_detections, count=None, overflow=0):
    """A GMTI slot as bytes: header (count, overflow, 0, 0), the reports, zeros up to max_detections reports."""
    reports = np.asarray(reports, REPORT_DTYPE)
    raw = np.zeros(16 + 48 * max_detections, np.uint8)
    raw[:8].view("<u4")[:] = (len(reports) if count is None else count, overflow)
    k = min(len(reports), max_detections)
    raw[16:16 + 48 * k] = reports[:k].view(np.uint8)
    return raw


def _terms(a, b, cells):
    """The terms of the four sums over `cells` of a = slc1, b = slc2 (complex64 [n_az x n_rg]): |a|^2, |b|^2, re and im of a conj(b)."""
    t11, t22, tre, tim = [], [], [], []
    for i, j in cells:
        ar, ai = float(a[i, j].real), float(a[i, j].imag)
        br, bi = float(b[i, j].real), float(b[i, j].imag)
        t11 += [ar * ar, ai * ai]
        t22 += [br * br, bi * bi]
        tre += [ar * br, ai * bi]
        tim += [ai * br, -(ar * bi)]
    return t11, t22, tre, tim


def _sum(terms):
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


class Result:
    """header: the four uint32 of the output header; reports: the kept reports (None after an overflow); stats: one STAT_DTYPE
    record per input report; abs: per report and sum, the sum of the absolute values of its terms; thr: k_sigma * sigma per report
    (nan where untested)."""

    def __init__(self, header, reports, stats, abs_terms, thr):
        self.header, self.reports, self.stats, self.abs, self.thr = np.asarray(header, "<u4"), reports, stats, abs_terms, thr
        self.n_kept = 0 if reports is None else len(reports)


def sums(reports, a, b, guard=(2, 2), train=(8, 8), looks=(1, 1)):
    """Steps 1 and 2 for every report: (stats with the six sums, n_train and n_look filled in, the sums of the absolute terms).
    The slow part; gate(..., sums_of=) takes it, so that one walk serves several parameter sets."""
    reports = np.asarray(reports, REPORT_DTYPE)
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    (ga, gr), (ta, tr), (la, lr) = guard, train, looks
    assert min(ga, gr, ta, tr) >= 0 and ga + ta <= MAX_HALF and gr + tr <= MAX_HALF and n_full(guard, train) >= 1
    assert 0 <= la <= min(MAX_LOOK, ga) and 0 <= lr <= min(MAX_LOOK, gr)
    n, (n_az, n_rg) = len(reports), a.shape
    oa, orr = ga + ta, gr + tr
    stats, abs_terms = np.zeros(n, STAT_DTYPE), np.zeros(n, ABS_DTYPE)
    for r in range(n):
        i, j = int(reports["i"][r]), int(reports["j"][r])
        ring, look = [], []
        if 0 <= i < n_az and 0 <= j < n_rg:
            for di in range(-oa, oa + 1):
                for dj in range(-orr, orr + 1):
                    if 0 <= i + di < n_az and 0 <= j + dj < n_rg:
                        if not (abs(di) <= ga and abs(dj) <= gr):
                            ring.append((i + di, j + dj))
                        if abs(di) <= la and abs(dj) <= lr:
                            look.append((i + di, j + dj))
        s = stats[r]
        t11, t22, tre, tim = _terms(a, b, ring)
        (s["c11"], abs_terms["c11"][r]), (s["c22"], abs_terms["c22"][r]) = _sum(t11), _sum(t22)
        (s["c12_re"], abs_terms["c12_re"][r]), (s["c12_im"], abs_terms["c12_im"][r]) = _sum(tre), _sum(tim)
        _, _, tre, tim = _terms(a, b, look)
        (s["i_re"], abs_terms["i_re"][r]), (s["i_im"], abs_terms["i_im"][r]) = _sum(tre), _sum(tim)
        s["n_train"], s["n_look"] = len(ring), len(look)
    return stats, abs_terms


def gate(reports, a, b, guard=(2, 2), train=(8, 8), looks=(1, 1), k_sigma=3.0, phase_min=0.0, min_coh=0.3, min_train=None,
         keep_untested=True, max_detections=None, count=None, overflow=0, sums_of=None):
    """a, b: complex64 [n_az x n_rg] (i = azimuth).  The semantics of include/sarx_atigate.h, step by step.  sums_of: what
    sums(reports, a, b, guard, train, looks) returned, when it has been formed already."""
    reports = np.asarray(reports, REPORT_DTYPE)
    if min_train is None:
        min_train = (n_full(guard, train) + 1) // 2
    md = max(len(reports), 1) if max_detections is None else int(max_detections)
    n = len(reports) if count is None else int(count)
    if overflow or n > md:
        return Result((n, 1, 0, 0), None, None, None, None)
    stats, abs_terms = sums(reports, a, b, guard, train, looks) if sums_of is None else (sums_of[0].copy(), sums_of[1])
    thr = np.full(n, np.nan)
    kept = []
    for r in range(n):
        s = stats[r]
        c11, c22, c12, big_i = float(s["c11"]), float(s["c22"]), complex(s["c12_re"], s["c12_im"]), complex(s["i_re"], s["i_im"])
        if s["n_train"] < min_train:
            s["reason"] = 1
        elif c11 * c22 == 0.0 or big_i == 0:
            s["reason"] = 2
        else:
            den = math.sqrt(c11 * c22)
            coh = min(math.hypot(c12.real / den, c12.imag / den), 1.0)
            s["coh"] = coh
            if coh < min_coh:
                s["reason"] = 3
            else:
                re = big_i.real * c12.real + big_i.imag * c12.imag
                im = big_i.imag * c12.real - big_i.real * c12.imag
                s["psi"] = math.atan2(im, re)
                with np.errstate(divide="ignore"):
                    s["sigma"] = float(np.sqrt(np.float64(1.0 - coh * coh) / np.float64(2.0 * int(s["n_look"]) * coh * coh)))
                thr[r] = k_sigma * float(s["sigma"])
                s["status"] = PASSED if abs(float(s["psi"])) > thr[r] and abs(float(s["psi"])) >= phase_min else REJECTED
        keep = s["status"] == PASSED or (s["status"] == UNTESTED and keep_untested)
        s["out_index"] = len(kept) if keep else -1
        if keep:
            kept.append(r)
    return Result((len(kept), 0, 0, 0), reports[:n][kept].copy(), stats, abs_terms, thr)


def decide(psi, sigma, k_sigma, phase_min):
    """Step 5 on arrays: thr = k_sigma * sigma, one rounded product; PASSED when |psi| > thr and |psi| >= phase_min."""
    psi, sigma = np.asarray(psi, np.float64), np.asarray(sigma, np.float64)
    with np.errstate(invalid="ignore"):
        thr = np.float64(k_sigma) * sigma
        return np.where((np.abs(psi) > thr) & (np.abs(psi) >= np.float64(phase_min)), PASSED, REJECTED)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
GRID = [(16 + 24 * p, 16 + 24 * q) for p in range(5) for q in range(5)]      # 25 places of a 128 x 128 image, 24 cells apart
SCENE_SEED = 7                                                               # the scene of tests/test_atigate.py and the GPU end-to-end test
MOVER_PHASES = (1.0, -1.5, 2.5, -3.0, 1.2)


def make_scene(seed, n_az=128, n_rg=128, coherence=0.9, n_static=8, mover_phases=MOVER_PHASES, amplitude=40.0, gain=1.12,
               mismatch_phase=0.06, clutter_phase=0.3, ramp=0.002):
    """Two co-registered images a = slc1, b = slc2 ([n_az x n_rg] complex64) and what was put into them:
      clutter   : c ~ CN(0, 1) common to both channels, plus independent noise CN(0, 1 / coherence - 1) in each, so the clutter's
                  coherence is `coherence`; channel 2 carries the clutter phase -(clutter_phase + ramp (i + j)): angle(a conj(b)) of
                  the clutter is clutter_phase plus a slow ramp
      statics   : n_static point scatterers of `amplitude`, channel 2 with the gain and phase mismatch gain e^{j mismatch_phase} on
                  top of the clutter phase: they leak through DPCA with amplitude |1 - gain e^{j mismatch_phase}|
      movers    : one point scatterer per entry of mover_phases, its ATI phase that many radians off the clutter's
    at places drawn from GRID (interior, 24 cells apart: no target lies in another's outer box of half-width 10).
    Returns a, b, dict(statics=[(i, j)], movers=[(i, j)], mover_phases=..., cal_phase=clutter_phase)."""
    rng = np.random.default_rng(seed)
    cn = lambda s: (rng.normal(size=(n_az, n_rg)) + 1j * rng.normal(size=(n_az, n_rg))) * math.sqrt(s / 2.0)
    c = cn(1.0)
    var = 1.0 / coherence - 1.0
    ii, jj = np.meshgrid(np.arange(n_az), np.arange(n_rg), indexing="ij")
    phi = clutter_phase + ramp * (ii + jj)
    a = c + cn(var)
    b = c * np.exp(-1j * phi) + cn(var)
    places = [g for g in GRID if g[0] < n_az - 10 and g[1] < n_rg - 10]
    pick = rng.permutation(len(places))[:n_static + len(mover_phases)]
    cells = [places[k] for k in pick]
    statics, movers = cells[:n_static], cells[n_static:]
    for (i, j) in statics:
        z = amplitude * np.exp(1j * rng.uniform(-np.pi, np.pi))
        a[i, j] += z
        b[i, j] += z * gain * np.exp(1j * mismatch_phase) * np.exp(-1j * phi[i, j])
    for (i, j), ph in zip(movers, mover_phases):
        z = amplitude * np.exp(1j * rng.uniform(-np.pi, np.pi))
        a[i, j] += z
        b[i, j] += z * np.exp(-1j * ph) * np.exp(-1j * phi[i, j])
    return a.astype(np.complex64), b.astype(np.complex64), dict(statics=sorted(statics), movers=sorted(movers),
                                                                 mover_phases=dict(zip(movers, mover_phases)), cal_phase=clutter_phase)


def parity_scene(seed, n_az, n_rg, coherence=0.8):
    """Clutter plus noise alone, every sample well away from zero in both channels' sum: what the parity tests put reports on."""
    a, b, _ = make_scene(seed, n_az, n_rg, coherence, n_static=0, mover_phases=())
    return a, b
