"""The step oracle of the four-step azimuth transform (tests/_az_steps_numpy.py) against the reference-pinned per-column helpers of
oracle/csa_oracle.py, and the teeth of the acceptance function tests/test_gpu_az_steps.py holds the device launches by: NumPy
"kernels" with one defect each, every one rejected with the offending row named.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _az_steps_numpy as az  # noqa: E402
from oracle import csa_oracle as orc  # noqa: E402

N_RG = 64
COLS = np.array([0, 1, 31, 32, 63])
# the plan's splits, and the swapped ones of the odd powers (slab mode's inverse)
SPLITS = [(n, S) for n, (S, RA) in az.PLAN_SPLITS.items()] + [(n, RA) for n, (S, RA) in az.PLAN_SPLITS.items() if RA != S]


def _args(n):
    return orc.focus_args(orc.scaled_radar(n, N_RG))


@pytest.mark.parametrize("n,S", SPLITS)
def test_forward_steps_compose_to_the_oracle_pass(n, S):
    x = az.noise(n, len(COLS), 1)
    args = _args(n)
    z = az.step_b(az.step_a(x, S), S, False, az.phi1_table(n, N_RG, COLS, args))
    assert orc.rel_l2(z, orc.azimuth_fft_cols(x, COLS, N_RG, *args)) < 1e-12


@pytest.mark.parametrize("n,S", SPLITS)
def test_inverse_steps_compose_to_the_oracle_pass(n, S):
    x = az.noise(n, len(COLS), 2)
    z = az.step_b(az.step_a(x, S, True), S, True)
    assert orc.rel_l2(z, orc.azimuth_ifft_cols(x)) < 1e-12


def test_impulse_rows_hit_every_residue():
    for n, (S, RA) in az.PLAN_SPLITS.items():
        r = az.impulse_rows(n, max(64, RA))
        assert len(set(r % S)) == S and len(set(r % RA)) == RA and len(set(r // S)) > 1
        x = az.impulses(n, max(64, RA))
        assert (np.count_nonzero(x, axis=0) == 1).all()
        # exact outputs: constant modulus on the step's support
        for sid, mod in ((az.FWD_A, 1.0), (az.INV_B, 1.0 / n)):
            y = np.abs(az.run_step(sid, x, S))
            assert np.allclose(y[y > 0.5 * mod], mod, rtol=1e-13) and not y[y <= 0.5 * mod].any()


@pytest.mark.parametrize("name", list(az.INPUTS))
@pytest.mark.parametrize("sid", az.STEP_IDS)
def test_the_complex64_comparator_is_accepted(sid, name):
    """a kernel as good as NumPy's complex64 transform passes every bound, on every input (ratio 1 by construction)"""
    n, (S, RA) = 2048, az.PLAN_SPLITS[2048]
    x = az.INPUTS[name](n, N_RG)
    phi = az.phi1_table(n, N_RG, np.arange(N_RG), _args(n))
    ref = az.run_step(sid, x, S, phi)
    got = az.run_step(sid, x, S, phi, dtype=np.complex64)
    e = az.accept(got, ref, got, f"{az.STEP_NAMES[sid]} {name}")
    assert e["ratio"] <= 1.0 and e["rel_l2"] < 1e-7 and e["col_l2"] < 1e-7


# ---- teeth: one defect each ------------------------------------------------------------------------------------------------------
def _rejected(got, ref, good, rows, check=None):
    with pytest.raises(az.StepMismatch) as ei:
        az.accept(got, ref, good, "defect")
    assert ei.value.row in rows, (ei.value.row, sorted(rows)[:8], str(ei.value))
    assert str(ei.value.row) in str(ei.value)
    if check:
        assert ei.value.check == check, str(ei.value)
    return ei.value


@pytest.mark.parametrize("n", [256, 16384])
@pytest.mark.parametrize("inverse", [False, True])
def test_teeth_one_twiddle_from_the_neighbouring_entry(n, inverse):
    """W_n^(q m' + 1) for one (q, m'): one row of 16384 is off by 2 pi / n = 3.8e-4 of itself, 3e-6 of the image - inside the
    whole-image bound, which is why the row bound exists."""
    S, RA = az.PLAN_SPLITS[n]
    x = az.noise(n, 8, 3)
    ref, good = az.step_a(x, S, inverse), az.step_a(x, S, inverse, np.complex64)
    q, m = S - 3, RA // 2 + 1
    tw = az.step_twiddle(n, S, inverse)
    tw[m, q] *= np.exp((2j if inverse else -2j) * np.pi / n)
    bad = az.step_a(x, S, inverse, np.complex64, twiddle=tw)
    err = _rejected(bad, ref, good, {q + m * S}, "row" if n == 16384 else None)
    if n == 16384:
        assert az.step_errors(bad, ref)["rel_l2"] < az.REL_L2_MAX          # the norm alone would have let it through
    az.accept(good, ref, good)
    assert err.row == q + m * S


@pytest.mark.parametrize("sid", az.STEP_IDS)
def test_teeth_two_output_bins_of_one_tile_exchanged(sid):
    n, (S, RA) = 2048, az.PLAN_SPLITS[2048]
    x = az.impulses(n, N_RG) + az.noise(n, N_RG, 4) * np.float32(1e-3)
    phi = az.phi1_table(n, N_RG, np.arange(N_RG), _args(n))
    ref, good = az.run_step(sid, x, S, phi), az.run_step(sid, x, S, phi, dtype=np.complex64)
    q = 5
    r1, r2 = (q + 3 * S, q + 4 * S) if sid in (az.FWD_A, az.INV_A) else (q + 3 * RA, q + 4 * RA)
    bad = good.copy()
    bad[[r1, r2], 32:] = good[[r2, r1], 32:]                                # the second 32-column tile only
    _rejected(bad, ref, good, {r1, r2})


def test_teeth_scale_of_one_tile():
    """1 / S instead of 1 / n in one tile of inverse step B"""
    n, (S, RA) = 1024, az.PLAN_SPLITS[1024]
    x = az.mixed_scale(n, N_RG, 5)
    ref, good = az.step_b(x, S, True), az.step_b(x, S, True, dtype=np.complex64)
    q = RA - 1
    bad = good.copy()
    bad[q::RA, :32] = good[q::RA, :32] * np.float32(n / S)
    _rejected(bad, ref, good, set(range(q, n, RA)))


def test_teeth_phi1_of_the_next_column_in_a_tile_s_last_column():
    n, (S, RA) = 4096, az.PLAN_SPLITS[4096]
    x = az.noise(n, N_RG, 6)
    args = _args(n)
    phi = az.phi1_table(n, N_RG, np.arange(N_RG), args)
    ref, good = az.step_b(x, S, False, phi), az.step_b(x, S, False, phi, np.complex64)
    phi_bad = phi.copy()
    phi_bad[:, 31] = phi[:, 32]
    bad = az.step_b(x, S, False, phi_bad, np.complex64)
    err = _rejected(bad, ref, good, set(range(n)))
    # one column in 64: the phase step between neighbouring columns decides which bound sees it; the worst place is in column 31
    e = az.step_errors(bad, ref)
    assert e["col_at"] == 31 and e["elem_at"][1] == 31 and err.row in (e["row_at"], e["elem_at"][0])


@pytest.mark.parametrize("inverse", [False, True])
def test_teeth_twiddle_sign_flipped_in_the_upper_half(inverse):
    n, (S, RA) = 512, az.PLAN_SPLITS[512]
    x = az.impulses(n, N_RG)
    ref, good = az.step_a(x, S, inverse), az.step_a(x, S, inverse, np.complex64)
    tw = az.step_twiddle(n, S, inverse)
    tw[:, S // 2:] = np.conj(tw[:, S // 2:])
    bad = az.step_a(x, S, inverse, np.complex64, twiddle=tw)
    _rejected(bad, ref, good, {q + m * S for q in range(S // 2, S) for m in range(1, RA)})


def test_teeth_leak_between_columns_of_different_scale():
    """1e-9 of the largest column added to every column: invisible in the whole-image norm, caught per column"""
    n, (S, RA) = 256, az.PLAN_SPLITS[256]
    x = az.mixed_scale(n, N_RG, 7)
    ref, good = az.step_b(x, S, True), az.step_b(x, S, True, dtype=np.complex64)
    big = int(np.argmax(np.abs(ref).max(axis=0)))
    bad = good + (np.float32(1e-9) * good[:, big])[:, None]
    assert az.step_errors(bad, ref)["rel_l2"] < 1e-7
    _rejected(bad, ref, good, set(range(n)))
