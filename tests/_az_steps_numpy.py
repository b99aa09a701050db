"""NumPy restatement of ONE launch of the four-step azimuth transform (az_step in csrc/api_csa.hip, sarx_csa_pass ids 110-113): the
checker of tests/test_az_steps.py and tests/test_gpu_az_steps.py.  complex128, numpy.fft only.

x is [n x cols], n = RA * S, q < S, m and m' < RA, W_k = exp(-2 pi i / k):

  step A forward (110)   y[q + m' S]   = W_n^(q m') * sum_m x[q + m S] W_RA^(m m')
  step A inverse (112)   the same with W -> conj(W), no scaling
  step B forward (111)   z[q' + m'' RA] = Phi1[q' + m'' RA, col] * sum_m y[q' S + m] W_S^(m m'')        (q' < RA, m'' < S)
  step B inverse (113)   conjugate kernels, times 1/n, no phase

S is a parameter: the plan uses 2^(floor(log2 n) / 2), slab mode splits the inverse the other way round (S <-> RA).

The complex64 form of the same step (dtype=np.complex64: numpy.fft keeps complex64 input complex64, the twiddles and Phi_1 are
rounded to complex64 before the multiply) sizes the element-wise bound of accept() and is never the expected value.  Its `twiddle`
and `phi1` arguments replace a table, which is how tests/test_az_steps.py builds kernels with one defect each."""
import numpy as np

from oracle import csa_oracle as orc

FWD_A, FWD_B, INV_A, INV_B = 110, 111, 112, 113
STEP_IDS = (FWD_A, FWD_B, INV_A, INV_B)
STEP_NAMES = {FWD_A: "fwd_A_twiddle", FWD_B: "fwd_B_phi1", INV_A: "inv_A_twiddle", INV_B: "inv_B_scale"}
# n_az -> (S, RA) as the plan splits it (az_s, api_csa.hip)
PLAN_SPLITS = {256: (16, 16), 512: (16, 32), 1024: (32, 32), 2048: (32, 64), 4096: (64, 64), 8192: (64, 128), 16384: (128, 128)}

REL_L2_MAX = 5e-6          # the project's bound for a whole azimuth pass at 16384^2; one step gets no more
ROW_MAX = 1e-5             # the per-row bound of test_mixed_radix_13200_range_passes
ELEM_FACTOR = 8.0          # worst element: at most this many times the complex64 NumPy comparator's own worst element
# What the comparator is charged at the least: an exact result of the column's RMS magnitude rounded once to complex64 (2^-24 per
# component).  It matters for the impulse inputs, where pocketfft adds zeros and can be exact to the last bit.
ELEM_FLOOR = np.sqrt(2.0) * 2.0 ** -24


def plan_split(n):
    return PLAN_SPLITS[n]


def step_twiddle(n, S, inverse=False):
    """[RA x S] table of W_n^(q m') at [m', q], complex128"""
    RA = n // S
    e = np.outer(np.arange(RA), np.arange(S)).astype(np.float64) / n
    return np.exp((2j if inverse else -2j) * np.pi * e)


def phi1_table(n_az, n_rg, cols, args):
    """Phi_1 at [azimuth bin, cols] as oracle.csa_oracle.azimuth_fft_cols builds it, in natural bin order (:272-274)"""
    lam, _, Kr, fs, prf, vr, r_ref, t0 = args
    tau, _, fa = orc.csa_axes(n_az, n_rg, fs, prf, t0)
    _, Cs, tau_ref = orc.migration_factors(fa, lam, vr, r_ref)
    tr = tau[np.asarray(cols)][None, :]
    return np.exp(-1j * np.pi * Kr * Cs[:, None] * (tr - tau_ref[:, None]) ** 2)


def _dft(x, axis, inverse):
    # norm="forward" leaves the inverse transform unscaled
    return np.fft.ifft(x, axis=axis, norm="forward") if inverse else np.fft.fft(x, axis=axis)


def step_a(x, S, inverse=False, dtype=np.complex128, twiddle=None):
    x = np.asarray(x, dtype=dtype)
    n, cols = x.shape
    RA = n // S
    tw = (step_twiddle(n, S, inverse) if twiddle is None else twiddle).astype(dtype)
    y = _dft(x.reshape(RA, S, cols), 0, inverse)                     # [m', q]
    assert y.dtype == dtype
    return (y * tw[:, :, None]).reshape(n, cols)                     # row q + m' S


def step_b(y, S, inverse=False, phi1=None, dtype=np.complex128, scale=None):
    """forward: `phi1` [n x cols] multiplies the result (None: plain transform); inverse: times `scale` (default 1/n)"""
    y = np.asarray(y, dtype=dtype)
    n, cols = y.shape
    RA = n // S
    z = _dft(y.reshape(RA, S, cols), 1, inverse)                     # [q', m'']
    assert z.dtype == dtype
    z = np.ascontiguousarray(z.transpose(1, 0, 2)).reshape(n, cols)  # row q' + m'' RA
    real = np.float32 if dtype == np.complex64 else np.float64
    if inverse:
        return z * real(1.0 / n if scale is None else scale)
    return z if phi1 is None else z * np.asarray(phi1).astype(dtype)


def run_step(step_id, x, S, phi1=None, dtype=np.complex128):
    if step_id == FWD_A:
        return step_a(x, S, False, dtype)
    if step_id == INV_A:
        return step_a(x, S, True, dtype)
    if step_id == FWD_B:
        return step_b(x, S, False, phi1, dtype)
    if step_id == INV_B:
        return step_b(x, S, True, None, dtype)
    raise ValueError(step_id)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def noise(n, cols, seed):
    r = np.random.default_rng([seed, n, cols])
    return (r.standard_normal((n, cols)) + 1j * r.standard_normal((n, cols))).astype(np.complex64)


def impulse_rows(n, cols):
    """Row of the one nonzero sample of each column: c * (n / cols + 1) mod n.  The factor is odd, so over any 2^k <= cols
    consecutive columns the rows hit every residue mod 2^k (mod S and mod RA once cols >= RA), while the row's high part walks
    through the whole extent."""
    g = n // cols + 1 if cols < n else 1
    assert g % 2 == 1
    return (np.arange(cols) * g) % n


def impulses(n, cols):
    x = np.zeros((n, cols), np.complex64)
    x[impulse_rows(n, cols), np.arange(cols)] = 1.0
    return x


def column_scales(cols, seed):
    s = 10.0 ** np.linspace(-6.0, 6.0, cols)
    return np.random.default_rng([seed, cols]).permutation(s)          # neighbouring columns differ by orders of magnitude


def mixed_scale(n, cols, seed):
    return (noise(n, cols, seed + 1) * column_scales(cols, seed)[None, :]).astype(np.complex64)


INPUTS = {"noise": lambda n, cols: noise(n, cols, 110), "impulses": impulses, "mixed_scale": lambda n, cols: mixed_scale(n, cols, 113)}


# ---- acceptance -----------------------------------------------------------------------------------------------------------------
class StepMismatch(AssertionError):
    """what accept() raises: .check names the bound, .row (and .col for the element bound) the worst place"""

    def __init__(self, msg, check, row, col=None):
        super().__init__(msg)
        self.check, self.row, self.col = check, row, col


def step_errors(got, ref):
    """got against the complex128 ref, over every row, column and element:
      rel_l2   ||got - ref|| / ||ref|| of the whole image          col_l2   the same per column, worst column
      row      max_r ||got[r] - ref[r]|| / ||ref[r]||               row_n    the same with every column divided by its RMS of ref first
      elem     max |got - ref| / (its column's RMS of ref)
    The column-normalised figures are what columns of very different scale are held by: in the plain ones the largest column
    hides the others."""
    ref = np.asarray(ref, dtype=np.complex128)
    d = np.abs(np.asarray(got).astype(np.complex128) - ref)
    assert d.shape == ref.shape and np.isfinite(d).all(), "shape mismatch or non-finite output"
    a = np.abs(ref)
    col_norm2 = np.sum(a ** 2, axis=0)
    assert (col_norm2 > 0).all()
    col_l2 = np.sqrt(np.sum(d ** 2, axis=0) / col_norm2)
    col_rms = np.sqrt(col_norm2 / ref.shape[0])
    dn = d / col_rms[None, :]
    row = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(a, axis=1), 1e-300)
    row_n = np.linalg.norm(dn, axis=1) / np.maximum(np.linalg.norm(a / col_rms[None, :], axis=1), 1e-300)
    worst = row if row.max() >= row_n.max() else row_n
    r, c = np.unravel_index(int(np.argmax(dn)), dn.shape)
    return {"rel_l2": float(np.sqrt(np.sum(d ** 2) / np.sum(col_norm2))), "col_l2": float(col_l2.max()), "col_at": int(col_l2.argmax()),
            "row": float(row.max()), "row_n": float(row_n.max()), "row_at": int(worst.argmax()),
            "elem": float(dn[r, c]), "elem_at": (int(r), int(c))}


def accept(got, ref, comparator, label=""):
    """The three bounds of a step result against the complex128 oracle `ref`; `comparator` is the complex64 NumPy result for the
    same input (or its step_errors figure `elem`).  Returns the figures (with `cmp_elem` and `ratio`); raises StepMismatch."""
    e = step_errors(got, ref)
    cmp_elem = float(comparator) if np.isscalar(comparator) else step_errors(comparator, ref)["elem"]
    e["cmp_elem"] = max(cmp_elem, ELEM_FLOOR)
    e["ratio"] = e["elem"] / e["cmp_elem"]
    if not max(e["rel_l2"], e["col_l2"]) <= REL_L2_MAX:
        raise StepMismatch(f"{label}: relative L2 {e['rel_l2']:.3e} (worst column {e['col_at']}: {e['col_l2']:.3e}) > {REL_L2_MAX:g}; "
                           f"worst row {e['row_at']}: {max(e['row'], e['row_n']):.3e}", "rel_l2", e["row_at"])
    if not max(e["row"], e["row_n"]) <= ROW_MAX:
        raise StepMismatch(f"{label}: row {e['row_at']} is off by {max(e['row'], e['row_n']):.3e} of its norm > {ROW_MAX:g}",
                           "row", e["row_at"])
    if not e["ratio"] <= ELEM_FACTOR:
        r, c = e["elem_at"]
        raise StepMismatch(f"{label}: element (row {r}, column {c}) is off by {e['elem']:.3e} of its column's RMS, "
                           f"{e['ratio']:.1f} x the complex64 comparator's {e['cmp_elem']:.3e} (> {ELEM_FACTOR:g} x)", "elem", r, c)
    return e
