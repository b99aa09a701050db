"""NumPy restatement of the GMTI detector's semantics (include/sarx_gmti.h, sarx/gmti.py): the checker of tests/test_gmti.py and
tests/test_gpu_gmti.py.  Written for clarity, not speed: the training sums are direct sums of non-negative terms (no
outer - guard difference), so they carry no cancellation of their own."""
import numpy as np


def n_full(guard, train):
    (ga, gr), (ta, tr) = guard, train
    return (2 * (ga + ta) + 1) * (2 * (gr + tr) + 1) - (2 * ga + 1) * (2 * gr + 1)


def cfar_alpha(pfa, n):
    return n * (pfa ** (-1.0 / n) - 1.0)


def _vsum(x, lo, hi):
    """y[i] = sum of x[i + d] for lo <= |d| <= hi (rows outside the image count as zero)"""
    n = x.shape[0]
    xp = np.zeros((n + 2 * hi,) + x.shape[1:], dtype=np.float64)
    xp[hi:hi + n] = x
    y = np.zeros(x.shape, dtype=np.float64)
    for d in range(-hi, hi + 1):
        if abs(d) >= lo:
            y += xp[hi + d:hi + d + n]
    return y


def _hsum(x, lo, hi):
    return _vsum(x.T, lo, hi).T


def _extent(idx, h, n):
    return np.minimum(idx + h, n - 1) - np.maximum(idx - h, 0) + 1


def cfar(m, guard=(2, 2), train=(8, 8), alpha=None, pfa=1e-6, min_train=None):
    """m: [n_az x n_rg] DPCA magnitude.  Returns dict: cells (sorted list of (i, j) reported), ratio (P / (alpha mean) per cell,
    nan where untested), mean, n_train, alpha."""
    (ga, gr), (ta, tr) = guard, train
    oa, orr = ga + ta, gr + tr
    nf = n_full(guard, train)
    if alpha is None:
        alpha = cfar_alpha(pfa, nf)
    if min_train is None:
        min_train = (nf + 1) // 2
    m = np.asarray(m, dtype=np.float32)
    n_az, n_rg = m.shape
    p = m.astype(np.float64) ** 2
    # T = {|di| <= oa, gr < |dj| <= orr}  +  {ga < |di| <= oa, |dj| <= gr}: two disjoint direct sums
    s = _hsum(_vsum(p, 0, oa), gr + 1, orr) + _hsum(_vsum(p, ga + 1, oa), 0, gr)
    ii = np.arange(n_az)[:, None]
    jj = np.arange(n_rg)[None, :]
    n_train = _extent(ii, oa, n_az) * _extent(jj, orr, n_rg) - _extent(ii, ga, n_az) * _extent(jj, gr, n_rg)
    mean = s / np.maximum(n_train, 1)
    tested = n_train >= min_train
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tested, p / (alpha * mean), np.nan)
    det = tested & (p > 0) & (p > alpha * mean)
    cells = []
    for i, j in zip(*np.nonzero(det)):
        mc = m[i, j]
        peak = True
        for di in range(-ga, ga + 1):
            for dj in range(-gr, gr + 1):
                if (di or dj) and 0 <= i + di < n_az and 0 <= j + dj < n_rg:
                    mq = m[i + di, j + dj]
                    if mq > mc or (mq == mc and (i + di) * n_rg + (j + dj) < i * n_rg + j):
                        peak = False
        if peak:
            cells.append((int(i), int(j)))
    return {"cells": sorted(cells), "ratio": ratio, "mean": mean, "n_train": n_train, "alpha": alpha, "power": p}


def interferogram(s1, s2, cells, cal_phase=0.0):
    """sum over the clipped 3 x 3 neighbourhood of slc1 conj(slc2 e^{j cal}) per cell, fp64 ([n_az x n_rg] images)."""
    s1 = np.asarray(s1, dtype=np.complex128)
    s2 = np.asarray(s2, dtype=np.complex128) * np.exp(1j * cal_phase)
    n_az, n_rg = s1.shape
    out = []
    for i, j in cells:
        a, b = slice(max(i - 1, 0), min(i + 2, n_az)), slice(max(j - 1, 0), min(j + 2, n_rg))
        out.append(np.sum(s1[a, b] * np.conj(s2[a, b])))
    return np.array(out, dtype=np.complex128)


def compare(cells_gpu, ref, band=1e-9):
    """(i, j) sets equal except cells whose ratio lies within `band` of 1.  Returns (missing, extra)."""
    g = set(map(tuple, cells_gpu))
    o = set(ref["cells"])
    r = ref["ratio"]
    near = lambda c: np.isfinite(r[c]) and abs(r[c] - 1.0) <= band
    return sorted(c for c in o - g if not near(c)), sorted(c for c in g - o if not near(c))
