"""The noise-pulse cases of tests/_tdbp_noise.py, checked on the CPU with the oracle alone: the conditions that make a case a case (the
census of the interpolation's classes at E-lo and E-hi), the tolerance against its cap, the agreement of the restated sample index
with the oracle's own, and the power of the per-pixel bar against three faults a back-projection kernel can have.

Why the per-pixel bar on noise exists beside the whole-image relative L2 < 1e-4 on point targets (figures of this module, 288
pulses, 33 x 17 pixels; "x bar" is the figure over its own bar):

    fault                                          noise, pixel_err (x tol)          point targets, rel L2 (x 1e-4)
                                                   N1              N2                N1             N2
    one compressed sample of one pulse zeroed      1.8e-2 (14)     2.9e-2 (250)      9.0e-5 (0.9)   1.2e-3 (12)
    one pulse's row shifted by one sample          1.1e-1 (84)     9.3e-2 (810)      6.4e-3 (64)    2.5e-2 (250)
    a ragged-tile pixel on pixel 0's coordinates   1.2e+0 (930)    3.9e+0 (34000)    9.1e-3 (91)    2.0e-3 (20)

The point-target scene is tb.tdbp_scene with three targets moving at vel_focus, on the same grid and pulses.  At this size the
whole-image bar is not blind to a shifted row or a misplaced pixel - a row shift costs about 2 / n_pulses of the image, far over 1e-4
at 288 pulses - but it sees every fault with a smaller margin than the per-pixel bar does, and a single lost sample, the kind of
fault a window that is one sample too narrow makes, with a margin at least ten times smaller: under its bar in N1.
test_bar_has_power asserts that ordering, and that each fault exceeds tol(case) on the noise pulses.
"""
import os
import sys

import numpy as np
import pytest

from oracle import tdbp_oracle as tb
from oracle.csa_oracle import rel_l2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_noise as tn  # noqa: E402

E_CASES = ["N1-lo", "N1-hi", "N2-lo", "N2-hi"]
ALL_CASES = ["N1", "N2"] + E_CASES + ["G1-row", "G1-col"]
CASES_AND_KINDS = [(n, "focus") for n in ALL_CASES] + [(n, "pair") for n in ALL_CASES + ["N1w"]]


@pytest.mark.parametrize("kind", ["focus", "pair"])
@pytest.mark.parametrize("name", E_CASES)
def test_edge_cases_reach_every_class_of_their_end(name, kind):
    """At least 100 (pulse, pixel) pairs in each of the three classes at that end, none at the other end, and the window bound of the
    host (floor(min idx_f) - 3, ceil(max idx_f) + 4) runs off that end, so the device clamps it."""
    c = tn.case(name, kind)
    n = c["num_samples"]
    for shift in ((False, True) if kind == "pair" else (False,)):
        cen = tn.index_census(c, shift)
        print(name, kind, shift, cen)
        if name.endswith("lo"):
            assert min(cen["below"], cen["lo_edge"], cen["inside"]) >= 100 and cen["hi_edge"] == cen["above"] == 0
            assert cen["i0_min"] < -1 and cen["idx_f_min"] < -3 and cen["i0_max"] < n - 1
        else:
            assert min(cen["inside"], cen["hi_edge"], cen["above"]) >= 100 and cen["below"] == cen["lo_edge"] == 0
            assert cen["i0_max"] >= n and cen["idx_f_max"] > n + 3 and cen["i0_min"] > 0


@pytest.mark.parametrize("kind", ["focus", "pair"])
@pytest.mark.parametrize("name", ["N1", "N2", "G1-row", "G1-col"])
def test_plain_cases_stay_inside_the_pulse(name, kind):
    cen = tn.index_census(tn.case(name, kind))
    assert cen["inside"] > 0 and cen["below"] == cen["lo_edge"] == cen["hi_edge"] == cen["above"] == 0
    if name == "N2" and kind == "focus":
        assert 110 < cen["i0_max"] - cen["i0_min"] < 130 and cen["i0_min"] < 560 < cen["i0_max"]


def test_case_shapes():
    n1, n2 = tn.case("N1"), tn.case("N2")
    assert (n1["num_samples"], int(n1["k"]["T_P"] * n1["k"]["FS"]), n2["num_samples"]) == (22004, 12000, 1122)
    assert n1["n_pulses"] == n2["n_pulses"] == 288 > 256 and (n1["nx"], n1["ny"]) == (33, 17)
    p = tn.noise_pulses(5, 7, 3)
    assert p.dtype == np.complex64 and p.shape == (5, 7) and np.array_equal(p, tn.noise_pulses(5, 7, 3))
    assert tn.pixel_err(np.array([1.0, 1.0 + 0.5j]), np.array([1.0, 1.0])) == pytest.approx(0.5)


@pytest.mark.parametrize("name,kind", CASES_AND_KINDS)
def test_floor_stays_under_the_cap(name, kind):
    """tol = 3 x the larger of the two measured floors must leave an eighth of one lost sample visible: 1 / (8 sqrt(n_pulses))."""
    c = tn.case(name, kind)
    for shift in ((False, True) if kind == "pair" else (False,)):
        f = tn.pixel_floor(c, shift)
        print(f"{name} {kind} shift={shift}: coord {f['coord']:.2e} rc {f['rc']:.2e} tol {f['tol']:.2e} cap {f['cap']:.2e}")
        assert 0.0 < f["tol"] < f["cap"] and f["tol"] == 3.0 * max(f["coord"], f["rc"])
    assert tn.cap(288) == pytest.approx(7.4e-3, rel=0.01)


def test_search_hypotheses_stay_under_the_cap():
    for name in ("N1", "N2", "N2-lo"):
        c = tn.case(name)
        for v in tn.search_hyps(c):
            f = tn.pixel_floor(tn.with_focus(c, v))
            assert 0.0 < f["tol"] < f["cap"]


def _capture_grid_sample(monkeypatch):
    seen = []
    real = tb._grid_sample_1d

    def spy(sig32, idx_norm, fused=True):
        seen.append(np.array(idx_norm, copy=True))
        return real(sig32, idx_norm, fused)
    monkeypatch.setattr(tb, "_grid_sample_1d", spy)
    return seen


@pytest.mark.parametrize("shift", [False, True])
def test_restated_pair_index_is_the_one_pair_images_interpolates_at(shift, monkeypatch):
    """Bit-equal input of _grid_sample_1d, both channels, on a tiny case: the first 12 pulses of N2-hi on 5 x 3 pixels."""
    c = dict(tn.case("N2-hi", "pair"))
    c.update(n_pulses=12, pos=c["pos"][:12], vel=c["vel"][:12], t_vec=c["t_vec"][:12], nx=5, ny=3)
    rc = [r[:12] for r in tn.rc_of(c)]
    seen = _capture_grid_sample(monkeypatch)
    tn.oracle_images(c, shift, rc=rc)
    assert len(seen) == 4                                             # real and imaginary plane of either channel
    for ch in range(2):
        mine = tn.idx_norm_of(c, tn.pair_idx_f(c, ch, shift))
        assert mine.shape == (12 - int(shift), 15)
        assert np.array_equal(mine, seen[2 * ch]) and np.array_equal(mine, seen[2 * ch + 1])


def test_restated_focus_index_is_the_one_the_oracle_interpolates_at(monkeypatch):
    c = dict(tn.case("N1-lo"))
    c.update(n_pulses=12, pos=c["pos"][:12], vel=c["vel"][:12], t_vec=c["t_vec"][:12], nx=5, ny=3)
    seen = _capture_grid_sample(monkeypatch)
    tn.oracle_images(c, rc=tn.rc_of(c)[:12])
    mine = tn.idx_norm_of(c, tn.focus_idx_f(c))
    assert len(seen) == 2 and np.array_equal(mine, seen[0]) and np.array_equal(mine, seen[1])
    x, i0 = tn.sample_position(mine, c["num_samples"])
    assert x.dtype == np.float32 and np.array_equal(i0, np.floor(x).astype(np.int64))


# ---- the power of the bar ------------------------------------------------------------------------------------------------------------

FAULT_PULSE = 147


def _faults(c, rc, image):
    """{fault: (faulty image, image)} of a focus case on compressed pulses rc.  The sample is the nearer tap of pixel (0, 0) - a
    corner, where a point-target scene has no energy - in pulse 147."""
    base = image(rc)
    x, i0 = tn.sample_position(tn.idx_norm_of(c, tn.focus_idx_f(c)), c["num_samples"])
    s = int(i0[FAULT_PULSE, 0]) + (1 if x[FAULT_PULSE, 0] - np.floor(x[FAULT_PULSE, 0]) >= 0.5 else 0)
    out = {}
    r = rc.copy(); r[FAULT_PULSE, s] = 0
    out["sample zeroed"] = (image(r), base)
    r = rc.copy(); r[FAULT_PULSE] = np.roll(rc[FAULT_PULSE], 1)
    out["row shifted"] = (image(r), base)
    f = base.copy(); f[5, c["nx"] - 1] = base[0, 0]                   # the one-pixel-wide tile column, run on pixel 0's coordinates
    out["pixel 0's coordinates"] = (f, base)
    return out


@pytest.mark.parametrize("name", ["N1", "N2"])
def test_bar_has_power(name):
    """Each fault exceeds tol(case) on the noise pulses.  On a point-target scene of the same shape (tb.tdbp_scene, three targets
    moving at vel_focus) the same faults stand over the whole-image 1e-4 bar by a far smaller factor, the single sample by less than
    2: see the table in the module docstring."""
    c = tn.case(name)
    tol = tn.pixel_floor(c)["tol"]
    noise = {k: tn.pixel_err(a, b) for k, (a, b) in _faults(c, tn.rc_of(c), lambda r: tn.oracle_images(c, rc=r)[0]).items()}
    vf = np.array(tn.VEL_FOCUS)
    sc = tb.tdbp_scene(n_pulses=c["n_pulses"], seed=5, k=c["k"], speed=float(np.linalg.norm(vf)), heading_deg=float(np.degrees(np.arctan2(vf[1], vf[0]))),
                       swath=c["swath"], n_targets=3)
    pc = dict(c)
    pc.update(t_start=sc["t_start"], vel_focus=sc["v_tgt"], pos=sc["pos"], vel=sc["vel"], t_vec=sc["t_vec"])
    rc = tb.range_compress(sc["raw"].astype(np.complex64), sc["num_samples"], sc["k"])
    point = {k: rel_l2(a, b) for k, (a, b) in _faults(pc, rc, lambda r: tn.oracle_images(pc, rc=r)[0]).items()}
    for k in noise:
        print(f"{name} {k}: noise pixel_err {noise[k]:.2e} = {noise[k] / tol:.0f} x tol {tol:.2e}; point targets rel L2 {point[k]:.2e} = {point[k] / 1e-4:.1f} x 1e-4")
        assert noise[k] > tol
        assert noise[k] / tol > point[k] / 1e-4
    assert noise["sample zeroed"] / tol > 10.0 * point["sample zeroed"] / 1e-4
