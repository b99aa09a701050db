"""NumPy restatement of the two-channel balance (include/sarx_balance.h, sarx/balance.py): the checker of tests/test_balance.py and
tests/test_gpu_balance.py.  fp64 throughout, written for clarity: block sums are plain np.sum over the block's kept pixels, the
per-pixel weight is the outer combination of the two axes' interpolation tables.  Images are [n_az x n_rg] (i = azimuth)."""
import numpy as np

F32_MAX = float(np.finfo(np.float32).max)


def n_blocks(n, block):
    return -(-int(n) // int(block))


def power_f32(s):
    """|s|^2 the way the header states the clip comparison: fp32 fmaf(re, re, im * im), im * im rounded to fp32 first."""
    s = np.asarray(s, dtype=np.complex64)
    re, im = s.real.astype(np.float64), s.imag
    with np.errstate(over="ignore", invalid="ignore"):
        return (re * re + (im * im).astype(np.float64)).astype(np.float32)


def kept(s1, s2, clip_power=np.inf):
    clip = np.float32(min(float(np.float32(clip_power)), F32_MAX))
    return (power_f32(s1) <= clip) & (power_f32(s2) <= clip)


def weight(s12, s11, s22, mode):
    """(w, coherence, usable) of one set of sums."""
    m = abs(s12)
    d = s11 * s22
    coh = m / np.sqrt(d) if d > 0 else 0.0
    if not (s22 > 0 and m > 0):
        return 1.0 + 0.0j, coh, False
    return (s12 / m if mode == "phase" else s12 / s22), coh, True


def estimate(s1, s2, block, mode="ls", clip_power=np.inf, min_count=1, min_coherence=0.0):
    """Block table of (s1, s2): dict of [nb_az x nb_rg] arrays s12, s11, s22, n, w, coherence, valid, and the global values."""
    s1 = np.asarray(s1, dtype=np.complex64).astype(np.complex128)
    s2 = np.asarray(s2, dtype=np.complex64).astype(np.complex128)
    n_az, n_rg = s1.shape
    ba, br = int(block[0]), int(block[1])
    nba, nbr = n_blocks(n_az, ba), n_blocks(n_rg, br)
    keep = kept(s1, s2, clip_power)
    t = {"s12": np.zeros((nba, nbr), np.complex128), "s11": np.zeros((nba, nbr)), "s22": np.zeros((nba, nbr)),
         "n": np.zeros((nba, nbr), np.int64), "w": np.zeros((nba, nbr), np.complex128), "coherence": np.zeros((nba, nbr)),
         "valid": np.zeros((nba, nbr), bool)}
    for a in range(nba):
        for r in range(nbr):
            sl = (slice(a * ba, min((a + 1) * ba, n_az)), slice(r * br, min((r + 1) * br, n_rg)))
            k = keep[sl]
            x, y = s1[sl][k], s2[sl][k]
            s12, s11, s22 = np.sum(x * np.conj(y)), float(np.sum(np.abs(x) ** 2)), float(np.sum(np.abs(y) ** 2))
            w, coh, ok = weight(s12, s11, s22, mode)
            t["s12"][a, r], t["s11"][a, r], t["s22"][a, r], t["n"][a, r] = s12, s11, s22, k.sum()
            t["w"][a, r], t["coherence"][a, r] = w, coh
            t["valid"][a, r] = ok and k.sum() >= min_count and coh >= min_coherence
    v = t["valid"]
    t["n_valid"] = int(v.sum())
    gw, gc, ok = weight(t["s12"][v].sum(), t["s11"][v].sum(), t["s22"][v].sum(), mode) if v.any() else (1.0 + 0.0j, 0.0, False)
    if not ok:
        gw, gc, t["n_valid"] = 1.0 + 0.0j, (gc if v.any() else 0.0), 0
    t["global_weight"], t["global_coherence"] = complex(gw), float(gc)
    t["w"] = np.where(v, t["w"], t["global_weight"])
    t["block"], t["shape"] = (ba, br), (n_az, n_rg)
    return t


def axis_table(n, block, interp="bilinear"):
    """b0, b1, f per index of an axis of n pixels cut into blocks of `block`."""
    nb = n_blocks(n, block)
    i = np.arange(n)
    if interp == "nearest":
        b = i // block
        return b, b, np.zeros(n)
    t = np.clip((i + 0.5) / block - 0.5, 0.0, nb - 1)
    b0 = np.minimum(np.floor(t).astype(np.int64), max(nb - 2, 0))
    return b0, np.minimum(b0 + 1, nb - 1), t - b0


def interpolate(table, shape, block, interp="bilinear"):
    """A [nb_az x nb_rg] table (complex or real; re and im go separately by linearity) on the pixel grid."""
    a0, a1, fa = axis_table(shape[0], block[0], interp)
    r0, r1, fr = axis_table(shape[1], block[1], interp)
    fa, fr = fa[:, None], fr[None, :]
    t = np.asarray(table)
    return (1 - fa) * ((1 - fr) * t[np.ix_(a0, r0)] + fr * t[np.ix_(a0, r1)]) + fa * ((1 - fr) * t[np.ix_(a1, r0)] + fr * t[np.ix_(a1, r1)])


def balance(s1, s2, block, mode="ls", interp="bilinear", clip_power=np.inf, min_count=1, min_coherence=0.0):
    """The whole product: the table (estimate), 'w_pixel', 'slc2' = w slc2 and 'dpca_mag' = |slc1 - slc2|, fp64."""
    t = estimate(s1, s2, block, mode, clip_power, min_count, min_coherence)
    s1 = np.asarray(s1, dtype=np.complex64).astype(np.complex128)
    s2 = np.asarray(s2, dtype=np.complex64).astype(np.complex128)
    t["w_pixel"] = interpolate(t["w"], s1.shape, t["block"], interp)
    t["slc2"] = t["w_pixel"] * s2
    t["dpca_mag"] = np.abs(s1 - t["slc2"])
    return t


# ---- the mismatch fixture: clutter common to both channels, a gain and phase mismatch no scalar follows, three movers ---------------
FIXTURE_SHAPE = (256, 192)
FIXTURE_MOVERS = (((77, 50), 1.0), ((140, 120), -2.0), ((200, 30), 0.7))       # (i, j), ATI phase
FIXTURE_MOVER_DB = 25.0
FIXTURE_CLIP = 10.0 ** 1.2
FIXTURE_BLOCK = (32, 32)


def mismatch_fixture(seed=7):
    n_az, n_rg = FIXTURE_SHAPE
    rng = np.random.default_rng(seed)

    def cn(power):
        return np.sqrt(power / 2) * (rng.standard_normal((n_az, n_rg)) + 1j * rng.standard_normal((n_az, n_rg)))
    c, n1, n2 = cn(1.0), cn(1e-3), cn(1e-3)
    i, j = np.arange(n_az)[:, None], np.arange(n_rg)[None, :]
    g = 1 + 0.2 * np.sin(2 * np.pi * i / n_az) * np.cos(np.pi * j / n_rg)
    phi = 0.6 * np.cos(2 * np.pi * j / n_rg) + 0.4 * i / n_az
    s1, s2 = c + n1, c + n2
    amp = 10.0 ** (FIXTURE_MOVER_DB / 20)
    for (mi, mj), p in FIXTURE_MOVERS:
        s1[mi, mj] += amp
        s2[mi, mj] += amp * np.exp(-1j * p)
    s2 = s2 / (g * np.exp(1j * phi))
    return s1.astype(np.complex64), s2.astype(np.complex64)


def mover_expected_db(p):
    return 10 * np.log10(abs(10.0 ** (FIXTURE_MOVER_DB / 20) * (1 - np.exp(-1j * p))) ** 2)


def residue_db(s1, s2b):
    """Mean DPCA power away from the movers (5 x 5 cells around each left out), over the unit clutter power."""
    d = np.abs(np.asarray(s1, np.complex128) - np.asarray(s2b, np.complex128)) ** 2
    m = np.ones(d.shape, bool)
    for (mi, mj), _ in FIXTURE_MOVERS:
        m[mi - 2:mi + 3, mj - 2:mj + 3] = False
    return 10 * np.log10(d[m].mean())


def mover_db(s1, s2b):
    return [10 * np.log10(abs(complex(s1[mi, mj]) - complex(s2b[mi, mj])) ** 2) for (mi, mj), _ in FIXTURE_MOVERS]
