"""NumPy restatement of the sliding-window coherence (include/sarx_coherence.h), the checker of tests/test_coherence.py and
tests/test_gpu_coherence*.py.  It reads nothing of the product.

Semantics restated.  a, b: complex64 [n_az x n_rg].  Window half-widths (ha, hr), each 0 .. 16: the window of pixel (i, j) is
|di| <= ha, |dj| <= hr clipped to the image, N(i, j) cells (a window larger than the image is allowed).  In fp64, from fp64 products
of the fp32 samples: S12 = sum a conj(b), S11 = sum |a|^2, S22 = sum |b|^2.  g = S12 / sqrt(S11 S22), 0 where S11 S22 = 0.
coh (fp32) = min(|g|, 1); igram (complex64) = g.  Change rule: tested = S11 >= power_floor N and S22 >= power_floor N; changed =
tested and the fp32 coh < (float)threshold; mask 0 = not tested, 1 = tested and unchanged, 2 = changed.  Summary: n_tested,
n_changed, sum_coh = the fp64 sum of the fp32 coh over the tested pixels.

Every window sum is a DIRECT sum of its terms (first the 2 ha + 1 rows, then the 2 hr + 1 columns of those): all additions, no
cumulative sum and no difference of sums, so nothing cancels."""
import numpy as np

MAX_HALF = 16


def _box(x, ha, hr):
    """Direct sum of x over the clipped window: shifted copies added one by one (zeros outside the image)."""
    n_az, n_rg = x.shape
    v = np.zeros_like(x)
    for d in range(-ha, ha + 1):
        lo, hi = max(0, -d), min(n_az, n_az - d)
        if lo < hi:
            v[lo:hi] += x[lo + d:hi + d]
    out = np.zeros_like(x)
    for d in range(-hr, hr + 1):
        lo, hi = max(0, -d), min(n_rg, n_rg - d)
        if lo < hi:
            out[:, lo:hi] += v[:, lo + d:hi + d]
    return out


def cells(n_az, n_rg, ha, hr):
    """N(i, j): the cells of the clipped window."""
    i, j = np.arange(n_az), np.arange(n_rg)
    ra = np.minimum(i + ha, n_az - 1) - np.maximum(i - ha, 0) + 1
    rr = np.minimum(j + hr, n_rg - 1) - np.maximum(j - hr, 0) + 1
    return ra[:, None] * rr[None, :]


def coherence(a, b, window, threshold=None, power_floor=0.0):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.complex64 and b.dtype == np.complex64 and a.shape == b.shape and a.ndim == 2
    ha, hr = window
    assert 0 <= ha <= MAX_HALF and 0 <= hr <= MAX_HALF
    ar, ai = a.real.astype(np.float64), a.imag.astype(np.float64)
    br, bi = b.real.astype(np.float64), b.imag.astype(np.float64)
    s12 = _box(ar * br, ha, hr) + _box(ai * bi, ha, hr) + 1j * (_box(ai * br, ha, hr) - _box(ar * bi, ha, hr))
    s11 = _box(ar * ar, ha, hr) + _box(ai * ai, ha, hr)
    s22 = _box(br * br, ha, hr) + _box(bi * bi, ha, hr)
    den = s11 * s22
    ok = den > 0
    g = np.zeros(a.shape, np.complex128)
    g[ok] = s12[ok] / np.sqrt(den[ok])
    coh = np.minimum(np.abs(g), 1.0).astype(np.float32)
    n = cells(a.shape[0], a.shape[1], ha, hr)
    out = {"g": g, "coh": coh, "igram": g.astype(np.complex64), "s11": s11, "s22": s22, "s12": s12, "n": n}
    thr = np.float32(0.0 if threshold is None else threshold)
    tested = (s11 >= power_floor * n) & (s22 >= power_floor * n)
    changed = tested & (coh < thr)
    out.update(tested=tested, changed=changed, mask=(tested.astype(np.uint8) + changed.astype(np.uint8)),
               n_tested=int(tested.sum()), n_changed=int(changed.sum()), sum_coh=float(coh[tested].astype(np.float64).sum()))
    return out


def clear_of_the_rule(r, threshold, power_floor, band=5e-7, rel=1e-12):
    """No pixel's coh within `band` of the threshold and no window sum within `rel` (relative) of power_floor N: then the mask and
    the counts do not depend on the last bits of the sums."""
    near_thr = np.abs(r["g"]).clip(max=1.0) - float(np.float32(threshold))
    if np.any(np.abs(near_thr) < band):
        return False
    need = power_floor * r["n"]
    for s in (r["s11"], r["s22"]):
        if np.any(np.abs(s - need) <= rel * np.maximum(np.abs(need), np.abs(s))) and power_floor > 0:
            return False
    return True


def speckle(shape, seed):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(shape) + 1j * r.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)


def pair(shape, kind, seed):
    """Seeded test pairs.  rho0 / rho05 / rho099: unit speckle of that correlation; phase: b = a e^{0.7j}; zeros: b = 0;
    patch: correlation 0.9 with a zero patch wider than any window in both images (and one in a alone); point: correlation 0.9 with
    one point target 80 dB above the speckle in power, in both images."""
    n_az, n_rg = shape
    a, w = speckle(shape, seed), speckle(shape, seed + 1000)
    rho = {"rho0": 0.0, "rho05": 0.5, "rho099": 0.99, "patch": 0.9, "point": 0.9}.get(kind)
    if kind == "phase":
        b = (a.astype(np.complex128) * np.exp(0.7j)).astype(np.complex64)
    elif kind == "zeros":
        b = np.zeros(shape, np.complex64)
    else:
        b = (rho * a.astype(np.complex128) * np.exp(0.3j) + np.sqrt(1 - rho * rho) * w).astype(np.complex64)
    if kind == "patch":
        i0, j0 = n_az // 4, n_rg // 5
        a[i0:i0 + 40, j0:j0 + 40] = 0
        b[i0:i0 + 40, j0:j0 + 40] = 0
        a[n_az // 2 + 3:n_az // 2 + 43, n_rg // 2:n_rg // 2 + 36] = 0
    if kind == "point":
        i0, j0 = (2 * n_az) // 3, n_rg // 3
        a[i0, j0] = 1e4
        b[i0, j0] = 1e4 * np.exp(0.3j)
    return a, b


def change_scene(seed=3):
    """96 x 80: a unit speckle, b = a e^{0.3j} + 0.1 of independent speckle, a 20 x 20 patch of b replaced by independent speckle.
    Returns (a, b, (i0, j0, size))."""
    shape = (96, 80)
    a = speckle(shape, seed)
    b = (a.astype(np.complex128) * np.exp(0.3j) + 0.1 * speckle(shape, seed + 1)).astype(np.complex64)
    i0, j0, size = 40, 30, 20
    b[i0:i0 + size, j0:j0 + size] = speckle((size, size), seed + 2)
    return a, b, (i0, j0, size)
