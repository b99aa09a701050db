"""NumPy restatement of the ordered-statistic CFAR's semantics (include/sarx_oscfar.h): the checker of tests/test_oscfar.py and
tests/test_gpu_oscfar.py.  Written for clarity: the decision of a cell is the count the header states, taken over the cell's
training set as a boolean mask over the clipped outer box; the level is the k-th smallest training power by np.partition.  All
arithmetic is fp64 on the exact P = m^2, so the device is held to it bit for bit."""
import numpy as np


def n_full(guard, train):
    (ga, gr), (ta, tr) = guard, train
    return (2 * (ga + ta) + 1) * (2 * (gr + tr) + 1) - (2 * ga + 1) * (2 * gr + 1)


def default_rank(guard, train):
    return (3 * n_full(guard, train)) // 4


def os_pfa(alpha, n, rank):
    """False-alarm rate of OS-CFAR for unit exponentials: prod_{i < rank} (n - i) / (n - i + alpha), as the plain product."""
    p = 1.0
    for i in range(rank):
        p *= (n - i) / (n - i + alpha)
    return p


def _extent(idx, h, n):
    return np.minimum(idx + h, n - 1) - np.maximum(idx - h, 0) + 1


def n_train(n_az, n_rg, guard, train):
    (ga, gr), (ta, tr) = guard, train
    ii, jj = np.arange(n_az)[:, None], np.arange(n_rg)[None, :]
    return _extent(ii, ga + ta, n_az) * _extent(jj, gr + tr, n_rg) - _extent(ii, ga, n_az) * _extent(jj, gr, n_rg)


def effective_rank(rank, n, nf):
    """k = ceil(rank n / N_full) in integers"""
    return (rank * n + nf - 1) // nf


def training_set(p, i, j, guard, train):
    """The powers of T(i, j): the outer box clipped to the image, minus the guard box (cells outside the image are not in it)."""
    (ga, gr), (ta, tr) = guard, train
    n_az, n_rg = p.shape
    i0, i1 = max(i - ga - ta, 0), min(i + ga + ta, n_az - 1) + 1
    j0, j1 = max(j - gr - tr, 0), min(j + gr + tr, n_rg - 1) + 1
    box = p[i0:i1, j0:j1]
    keep = np.ones(box.shape, bool)
    keep[max(i - ga, 0) - i0:min(i + ga, n_az - 1) + 1 - i0, max(j - gr, 0) - j0:min(j + gr, n_rg - 1) + 1 - j0] = False
    return box[keep]


def peaks(m, guard):
    """The peak rule of sarx_gmti.h for every cell: no cell of the guard box inside the image is larger, and no equal one has a
    smaller linear index."""
    ga, gr = guard
    n_az, n_rg = m.shape
    ok = np.ones(m.shape, bool)
    for di in range(-ga, ga + 1):
        for dj in range(-gr, gr + 1):
            if not di and not dj:
                continue
            if abs(di) >= n_az or abs(dj) >= n_rg:
                continue                                          # that neighbour is outside the image for every cell
            a = slice(max(-di, 0), n_az - max(di, 0))             # cells whose neighbour (i + di, j + dj) is inside
            b = slice(max(-dj, 0), n_rg - max(dj, 0))
            an = slice(max(di, 0), n_az - max(-di, 0))
            bn = slice(max(dj, 0), n_rg - max(-dj, 0))
            mc, mq = m[a, b], m[an, bn]
            first = di < 0 or (di == 0 and dj < 0)
            ok[a, b] &= ~((mq > mc) | ((mq == mc) & first))
    return ok


def oscfar(m, guard=(2, 2), train=(8, 8), alpha=None, rank=None, min_train=None, every_cell=False):
    """m: [n_az x n_rg] DPCA magnitude (>= 0).  Returns dict: cells (sorted (i, j) reported), power / level (fp64 per reported
    cell, in that order), n_train, k (per cell), peak, tested, and for the cells that were evaluated count (#{alpha P_t < P}),
    level_map (x_(k); nan elsewhere) and detected.  Evaluated are the tested cells with P > 0 that pass the peak rule - the only
    ones that can be reported - or, with every_cell=True, all tested cells."""
    nf = n_full(guard, train)
    rank = default_rank(guard, train) if rank is None else int(rank)
    assert 1 <= rank <= nf and alpha is not None and alpha > 0
    if min_train is None:
        min_train = (nf + 1) // 2
    m = np.asarray(m, dtype=np.float32)
    n_az, n_rg = m.shape
    p = m.astype(np.float64) ** 2
    nt = n_train(n_az, n_rg, guard, train)
    k = effective_rank(rank, nt, nf)
    tested = nt >= min_train
    peak = peaks(m, guard)
    todo = tested if every_cell else tested & peak & (p > 0)
    count = np.full(m.shape, -1, np.int64)
    level = np.full(m.shape, np.nan)
    for i, j in zip(*np.nonzero(todo)):
        t = training_set(p, i, j, guard, train)
        assert t.size == nt[i, j]
        count[i, j] = np.count_nonzero(alpha * t < p[i, j])       # one fp64 product per cell, strict
        level[i, j] = np.partition(t, k[i, j] - 1)[k[i, j] - 1]
    detected = todo & (p > 0) & (count >= k)
    rep = detected & peak
    cells = sorted((int(i), int(j)) for i, j in zip(*np.nonzero(rep)))
    ii = np.array([c[0] for c in cells], dtype=np.int64)
    jj = np.array([c[1] for c in cells], dtype=np.int64)
    return {"cells": cells, "power": p[ii, jj] if cells else np.zeros(0), "level": level[ii, jj] if cells else np.zeros(0),
            "n_train": nt, "k": k, "peak": peak, "tested": tested, "count": count, "level_map": level, "detected": detected,
            "evaluated": todo, "p": p, "alpha": alpha, "rank": rank}


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
MASKING_CELLS = [(48, 20), (48, 27), (48, 34), (48, 41), (48, 48), (24, 60), (30, 64), (24, 68)]
MASKING_DB = [40, 18, 40, 18, 40, 18, 40, 18]


def masking_scene(seed=20261019):
    """96 x 96 unit-mean exponential power with 18 dB movers inside the training windows of 40 dB ones."""
    rng = np.random.default_rng(seed)
    m = np.sqrt(rng.exponential(1.0, (96, 96))).astype(np.float32)
    for (i, j), db in zip(MASKING_CELLS, MASKING_DB):
        m[i, j] = 10.0 ** (db / 20.0)
    return m


def speckle_plane(shape, seed, db=(25.0, 45.0)):
    """Unit-mean exponential power with planted targets: one in a corner, one on each border, the others anywhere, among them two
    equal neighbours (the tie rule)."""
    n_az, n_rg = shape
    rng = np.random.default_rng(seed)
    m = np.sqrt(rng.exponential(1.0, shape)).astype(np.float32)
    spots = [(0, 0), (0, n_rg // 2), (n_az - 1, n_rg // 3), (n_az // 2, 0), (n_az // 3, n_rg - 1), (n_az - 1, n_rg - 1)]
    k = max(4, n_az * n_rg // 600)
    spots += list(zip(rng.integers(0, n_az, k).tolist(), rng.integers(0, n_rg, k).tolist()))
    for i, j in spots:
        m[i, j] = 10.0 ** (rng.uniform(*db) / 20.0)
    i, j = spots[-1]
    m[i, min(j + 1, n_rg - 1)] = m[i, j]
    return m


def quantised_plane(shape, seed):
    """m in {1, 2, 4} with probabilities 0.6, 0.3, 0.1: with alpha = 4 every cell of m = 2 whose k-th smallest training power is 1
    has alpha x_(k) == P exactly."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([1.0, 2.0, 4.0], np.float32), size=shape, p=[0.6, 0.3, 0.1])
