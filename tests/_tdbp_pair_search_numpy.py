"""fp64 NumPy restatement of the focus-velocity search on the two-receiver back-projection (include/sarx_tdbp_pair_search.h).
TEST INFRASTRUCTURE ONLY.

Written from the header on the arithmetic of tests/_tdbp_pair_numpy.pair_images, evaluated on the chip's pixels alone: the grid
axes are the full linspace of the grid, then sliced.  Records, k_best and the interferogram are plain NumPy.  It also fixes the
long scene that tests/test_tdbp_pair_search.py (physics, CPU) and tests/test_gpu_tdbp_pair_search.py (end to end, GPU) share."""
import functools

import numpy as np

from oracle import tdbp_oracle as tb

import _tdbp_pair_numpy as pref

DPCA, CH0 = "dpca", "ch0"


def chip_origin(i, j, nx, ny, chip_x, chip_y):
    """(x0, y0) of the chip around report (i, j) = (row iy, column ix), or None for a report outside the grid."""
    if not (0 <= i < ny and 0 <= j < nx):
        return None
    return int(np.clip(j - chip_x // 2, 0, nx - chip_x)), int(np.clip(i - chip_y // 2, 0, ny - chip_y))


def chip_images(sc, scene_size, nx, ny, shift, x0, y0, chip_x, chip_y, vel_focus):
    """complex128 [2 x chip_y x chip_x]: both channels at the grid pixels [y0, y0 + chip_y) x [x0, x0 + chip_x)."""
    k = sc["k"]
    C, FC, FS, n_s = k["C"], k["FC"], k["FS"], sc["num_samples"]
    if "rc" not in sc:
        sc["rc"] = [tb.range_compress(r, n_s, k) for r in sc["raw"]]
    first, n_used = shift if not isinstance(shift, bool) else pref.pulse_ranges(len(sc["t_vec"]), shift)
    pos, vel, t_p = (np.asarray(sc[n], dtype=np.float64) for n in ("pos", "vel", "t_vec"))
    dt_all = t_p - np.mean(t_p)                                       # over ALL pulses
    v_hat = vel / np.linalg.norm(vel, axis=1, keepdims=True)
    v_f = np.asarray(vel_focus, dtype=np.float64).reshape(1, 1, 3)
    xs = np.linspace(-scene_size / 2, scene_size / 2, nx)[x0:x0 + chip_x]
    ys = np.linspace(-scene_size / 2, scene_size / 2, ny)[y0:y0 + chip_y]
    gx, gy = np.meshgrid(xs, ys, indexing="xy")
    grid = np.stack((gx.ravel(), gy.ravel(), np.zeros(gx.size)), axis=1)
    out = np.zeros((2, grid.shape[0]), dtype=np.complex128)
    for c in range(2):
        sl = slice(first[c], first[c] + n_used)
        re32 = np.ascontiguousarray(sc["rc"][c].real.astype(np.float32)[sl])
        im32 = np.ascontiguousarray(sc["rc"][c].imag.astype(np.float32)[sl])
        p_tx = pos[sl][:, None, :]
        p_rx = p_tx + sc["rx_offsets"][c] * v_hat[sl][:, None, :]
        g = grid[None, :, :] + v_f * dt_all[sl].reshape(-1, 1, 1)
        tau = (np.linalg.norm(g - p_tx, axis=2) + np.linalg.norm(g - p_rx, axis=2)) / C
        idx_norm = 2 * ((tau - sc["t_start"] + sc["chirp_centre"]) * FS) / n_s - 1
        s = tb._grid_sample_1d(re32, idx_norm).astype(np.float64) + 1j * tb._grid_sample_1d(im32, idx_norm).astype(np.float64)
        out[c] = np.sum(s * np.exp(1j * (2 * np.pi * FC * tau)), axis=0)
    return out.reshape(2, chip_y, chip_x)


def power(chip, source):
    """P = re(D)^2 + im(D)^2 of one chip [2 x chip_y x chip_x], two rounded products and one rounded sum."""
    d = chip[0] - chip[1] if source == DPCA else chip[0]
    return d.real * d.real + d.imag * d.imag


def record(chip, x0, y0, source):
    """(s2, s4, peak, peak_ix, peak_iy) of one chip; grid coordinates; of equal maxima the first in row-major order; NaN never the peak."""
    p = power(chip, source)
    if np.isnan(p).all():
        return float(np.sum(p)), float(np.sum(p * p)), float("nan"), -1, -1
    at = int(np.nanargmax(p.ravel()))                                 # argmax returns the first of equal maxima
    return float(np.sum(p)), float(np.sum(p * p)), float(p.ravel()[at]), x0 + at % p.shape[1], y0 + at // p.shape[1]


def best(chips, x0, y0, source):
    """The best record of one report from its chips [n_hyp x 2 x chip_y x chip_x]: a dict of the header's fields and `records`."""
    recs = [record(c, x0, y0, source) for c in chips]
    s4 = np.array([r[1] for r in recs])
    kb = 0
    for h in range(1, len(s4)):
        if s4[h] > s4[kb] or (np.isnan(s4[kb]) and not np.isnan(s4[h])):
            kb = h
    _, _, _, ix, iy = recs[kb]
    out = dict(k_best=kb, x0=x0, y0=y0, peak_ix=ix, peak_iy=iy, s4_prev=s4[kb - 1] if kb > 0 else -1.0, s4_best=s4[kb],
               s4_next=s4[kb + 1] if kb + 1 < len(s4) else -1.0, records=recs)
    c = chips[kb]
    cy, cx = iy - y0, ix - x0
    a = c[0, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2]
    b = c[1, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2]
    out["interf"] = complex(np.sum(a * np.conj(b)))
    out["interf_scale"] = float(np.sum(np.abs(a) * np.abs(b)))
    out["p0"], out["p1"] = float(abs(c[0, cy, cx]) ** 2), float(abs(c[1, cy, cx]) ** 2)
    return out


def search(sc, scene_size, nx, ny, shift, reports, vel_hyps, chip, source=DPCA):
    """Per report (i, j): None outside the grid, else best() with `chips` [n_hyp x 2 x chip_y x chip_x] added."""
    chip_x, chip_y = chip
    out = []
    for i, j in reports:
        o = chip_origin(int(i), int(j), nx, ny, chip_x, chip_y)
        if o is None:
            out.append(None)
            continue
        chips = np.stack([chip_images(sc, scene_size, nx, ny, shift, o[0], o[1], chip_x, chip_y, v) for v in vel_hyps])
        b = best(chips, o[0], o[1], source)
        b["chips"] = chips
        out.append(b)
    return out


# the long scene of the issue: the data carry the along-track speed only over a long aperture
LONG_PULSES = 2048
LONG_MOVER_V = (9.0, 10.0, 0.0)            # along track 9 m/s (what the search finds), ground range 10 m/s (what ATI finds)
LONG_GRID = (90, 70, 360.0)                # nx, ny, scene size
LONG_PEAK = (36, 45)                       # (iy, ix) of the DPCA peak with vel_focus = 0
STRONG = (14.0, -4.0, 5000.0)              # a stationary scatterer inside the 24 x 24 chip around that peak


@functools.lru_cache(maxsize=None)
def long_scene(strong=False):
    """Six stationary scatterers (and the strong one on request) and a mover at (495, 0) m with velocity (9, 10, 0) m/s, 2048 pulses."""
    stat = pref.six_scatterers() + ([STRONG] if strong else [])
    return pref.scene(LONG_PULSES, tb.scaled_constants(), stat, [(pref.MOVER_AT[0], pref.MOVER_AT[1], 50.0, LONG_MOVER_V)])


def along_track_line(offsets):
    """Focus velocities (9 + s, 0, 0) m/s: the radial component left at zero (a mismatch there displaces, it does not defocus)."""
    return np.array([[LONG_MOVER_V[0] + s, 0.0, 0.0] for s in offsets])
