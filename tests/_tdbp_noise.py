"""Noise-pulse cases for the per-pixel back-projection tests (tests/test_tdbp_pixelwise.py on the CPU, tests/test_gpu_tdbp_pixelwise.py on
the GPU).  TEST INFRASTRUCTURE ONLY.

A point-target scene puts the image's energy into a few dozen pixels, and a relative L2 over the whole image sees nothing else.  Here
the pulses are complex Gaussian noise: every compressed sample matters to the pixels that read it, every pixel has comparable
magnitude, and ``t_start`` is free, since nothing ties the samples to the geometry - a scene can be slid onto either end of the pulse,
where the zero padding of the interpolation is.

The module holds the cases (N1, N2, their E-lo / E-hi forms, G1), the restated sample index of oracle.tdbp_oracle.tdbp and of
tests/_tdbp_pair_numpy.pair_images with a census of its classes, the per-pixel error measure and the per-pixel tolerance, which is
measured on the oracle alone (``pixel_floor``): nothing here knows the device.
"""
import functools

import numpy as np

from oracle import tdbp_oracle as tb

import _tdbp_pair_numpy as pref

NX, NY = 33, 17                       # 3 x 2 tiles of 16 x 16: a one-pixel-wide ragged tile column, a one-pixel-high ragged tile row
VEL_FOCUS = (3.0, -2.0, 0.0)
N_PULSES = 288                        # crosses the 256-pulse batch of the tile form
SEED, SEED_PAIR, SEED_STALE, SEED_FLOOR = 101, (211, 223), 307, 401
COORD_SHIFT = 1e-6                    # samples: the coordinate error the tile form documents (csrc/tdbp_pixel.hpp)
RC_REL_L2 = 1e-5                      # the bar tests/test_gpu_tdbp.py::test_range_compression_matches_oracle holds rc to
MARGIN = 3.0
# E-lo / E-hi.  An image row is a line of constant ground range: over its 33 pixels and 288 pulses idx_f moves by 0.1 to 0.4 sample,
# and from row to row by 4.5 to 7.5.  The classes of i0 therefore come in whole rows of 9504 pairs, and a rule on the extreme idx_f
# alone (say "the smallest is -4") puts a whole row into one class and none into the next.  The rule here is on a quantile: the
# median of the second row from that end sits on the class boundary (idx_f = -0.5 between i0 = -2 and i0 = -1; idx_f = n_s + 0.5
# between i0 = n_s - 1 and i0 = n_s).  Half of that row reads one padded tap, the other half and the whole outermost row (idx_f about
# -7 or n_s + 7) read two, so that row of the image is exactly zero, and every other row lies inside.
E_QUANTILE = 1.5 / NY

RADARS = {"native": tb.batch_constants, "scaled": tb.scaled_constants}
BASES = {                             # radar, scene size [m]: N1 metre-sized pixels (tile route), N2 12.5 x 25 m pixels (exact route)
    "N1": ("native", 33.0),
    "N2": ("scaled", 400.0),
    "N1w": ("native", 33.0),          # pair only, see PAIR_SWATH
}
# The pair's tile form has a bound of its own beside the focus's (csrc/tdbp_pair.hip, pair_bounds): |q|^2 |off| / (sqrt(3) d^2) < 1e-9 m
# with q the tile's reach, 8 hypot(swath / 32, swath / 16) on this grid, |off| = V / PRF = 1.54 m and d = 5.1e5 m.  At 33 m that is
# 1.2e-9 m, so the pair takes the exact kernel there (case N1w holds it to that); at 24 m it is 6e-10 m, and that is the pair's N1.
PAIR_SWATH = {"N1": 24.0}


def noise_pulses(n_p, n_s, seed):
    """complex64 [n_p x n_s], real and imaginary parts standard normal."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_p, n_s), dtype=np.float32) + 1j * rng.standard_normal((n_p, n_s), dtype=np.float32)).astype(np.complex64)


def pixel_err(img, ref):
    """max |img - ref| / rms(|ref|)."""
    img, ref = np.asarray(img, dtype=np.complex128), np.asarray(ref, dtype=np.complex128)
    return float(np.max(np.abs(img - ref)) / np.sqrt(np.mean(np.abs(ref) ** 2)))


def cap(n_pulses):
    """An eighth of what one lost sample does to one pixel of a noise image: a condition on the tolerance, not a measurement."""
    return 1.0 / (8.0 * np.sqrt(n_pulses))


# ---- the cases ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pulses(radar, seed):
    return noise_pulses(N_PULSES, tb.spotlight_window(RADARS[radar]())[0], seed)


@functools.lru_cache(maxsize=None)
def _compressed(radar, seed):
    k = RADARS[radar]()
    return tb.range_compress(_pulses(radar, seed), tb.spotlight_window(k)[0], k)


def _case(base, kind, nx=NX, ny=NY):
    radar, swath = BASES[base]
    k = RADARS[radar]()
    if kind == "pair":
        swath = PAIR_SWATH.get(base, swath)
    n_s, t_start, _ = tb.spotlight_window(k)
    t_vec = (np.arange(N_PULSES) - N_PULSES / 2) / k["PRF"]
    pos, vel = tb.orbit_arc(t_vec, k)
    c = dict(name=base, base=base, radar=radar, kind=kind, k=k, swath=swath, nx=nx, ny=ny, num_samples=n_s, t_start=t_start, t_vec=t_vec, pos=pos,
             vel=vel, vel_focus=np.array(VEL_FOCUS), n_pulses=N_PULSES)
    if kind == "pair":
        speed = float(np.linalg.norm(vel[N_PULSES // 2]))
        c.update(rx_offsets=(-speed / k["PRF"], speed / k["PRF"]), chirp_centre=k["T_P"] / 2, seeds=SEED_PAIR)
    else:
        c.update(seeds=(SEED,))
    return c


def _slide(c, end):
    """The same case with t_start moved until the scene reads off the low or the high end of the pulse (idx_f is linear in t_start)."""
    idx = np.concatenate([i.ravel() for i in all_idx_f(c)])
    d = (np.quantile(idx, E_QUANTILE) + 0.5) if end == "lo" else (np.quantile(idx, 1.0 - E_QUANTILE) - (c["num_samples"] + 0.5))
    e = dict(c)
    e.update(name=f"{c['name']}-{end}", t_start=c["t_start"] + d / c["k"]["FS"])
    return e


@functools.lru_cache(maxsize=None)
def case(name, kind="focus"):
    """name: N1, N2, N1-lo, N1-hi, N2-lo, N2-hi, G1-row (17 x 1 pixels of N2), G1-col (1 x 17), N1w (pair only); kind: "focus" (also the search's) or
    "pair" (two channels, receivers at -+ V / PRF, chirp centre T_P / 2; slid with every pulse in use).  Treat the dict as read-only."""
    base, _, end = name.partition("-")
    if base == "G1":
        c = _case("N2", kind, *((17, 1) if end == "row" else (1, 17)))
        c["name"] = name
        return c
    c = _case(base, kind)
    return _slide(c, end) if end else c


def with_focus(c, vel_focus):
    """The same case under another focus velocity (a hypothesis of the search)."""
    e = dict(c)
    e.update(vel_focus=np.asarray(vel_focus, dtype=np.float64), name=f"{c['name']}@{tuple(float(v) for v in vel_focus)}")
    return e


def raw_of(c):
    """The pulses of a case: one array for a focus case, the two channels for a pair."""
    r = [_pulses(c["radar"], s) for s in c["seeds"]]
    return r if c["kind"] == "pair" else r[0]


def rc_of(c):
    """oracle.tdbp_oracle.range_compress of raw_of(c), computed once per realisation."""
    r = [_compressed(c["radar"], s) for s in c["seeds"]]
    return r if c["kind"] == "pair" else r[0]


def stale_pulses(c):
    """Another realisation, 1000 times as large: what a plan's compressed buffer is filled with before the windowed focus."""
    return (1000.0 * _pulses(c["radar"], SEED_STALE)).astype(np.complex64)


def search_scene(c):
    """The case as the dict tests/_tdbp_search_numpy.stack_images takes."""
    return dict(raw=raw_of(c), pos=c["pos"], vel=c["vel"], t_start=c["t_start"], num_samples=c["num_samples"], t_vec=c["t_vec"],
                swath=c["swath"], k=c["k"])


def search_hyps(c):
    return np.array([np.zeros(3), c["vel_focus"], c["vel_focus"] + np.array([6.0, -0.2, 0.0])])


# ---- the oracle's images of a case ---------------------------------------------------------------------------------------------

def oracle_images(c, shift=False, t_start=None, rc=None):
    """complex128 [n_img x ny x nx]: one image of a focus case, the two channels of a pair."""
    t_start = c["t_start"] if t_start is None else t_start
    rc = rc_of(c) if rc is None else rc
    if c["kind"] == "pair":
        first, n_used = pref.pulse_ranges(c["n_pulses"], shift)
        return pref.pair_images(raw_of(c), c["pos"], c["vel"], c["t_vec"], t_start, c["num_samples"], c["swath"], c["nx"], c["ny"], c["k"],
                                c["rx_offsets"], c["chirp_centre"], first, n_used, c["vel_focus"], rc=rc)
    return tb.tdbp(None, c["pos"], c["vel"], t_start, c["num_samples"], c["vel_focus"], c["t_vec"], c["swath"], c["nx"], c["ny"], c["k"],
                   rc_data=rc)[None]


# ---- the sample index, restated -------------------------------------------------------------------------------------------------

def _grid(c):
    s = c["swath"]
    gx, gy = np.meshgrid(np.linspace(-s / 2, s / 2, c["nx"]), np.linspace(-s / 2, s / 2, c["ny"]), indexing="xy")
    return np.stack((gx.ravel(), gy.ravel(), np.zeros(gx.size)), axis=1)


def focus_idx_f(c, t_start=None):
    """idx_f [n_pulses x n_pix] of oracle.tdbp_oracle.tdbp (sar_batch_sim.py:205-221), operation for operation."""
    k = c["k"]
    C, FC, FS, K_RATE = k["C"], k["FC"], k["FS"], k["K_RATE"]
    t_start = c["t_start"] if t_start is None else t_start
    pos, vel = np.asarray(c["pos"], dtype=np.float64), np.asarray(c["vel"], dtype=np.float64)
    v_f = np.asarray(c["vel_focus"], dtype=np.float64).reshape(1, 1, 3)
    t_p = np.asarray(c["t_vec"], dtype=np.float64).reshape(-1, 1, 1)
    g = _grid(c)[None, :, :] + v_f * (t_p - np.mean(t_p))
    d_tx_v = g - pos[:, None, :]
    d_tx = np.linalg.norm(d_tx_v, axis=2)
    v_rad = np.sum((vel[:, None, :] - v_f) * (d_tx_v / d_tx[:, :, None]), axis=2)
    t_shift = (-FC * (2 * v_rad / C)) / K_RATE
    tau_a = 2 * d_tx / C
    d_rx = np.linalg.norm((g + v_f * tau_a[:, :, None]) - (pos[:, None, :] + vel[:, None, :] * tau_a[:, :, None]), axis=2)
    tau = (d_tx + d_rx) / C
    return (tau - t_start + t_shift) * FS


def pair_idx_f(c, chan, shift=False, t_start=None):
    """idx_f [n_used x n_pix] of channel chan of tests/_tdbp_pair_numpy.pair_images, operation for operation."""
    k = c["k"]
    t_start = c["t_start"] if t_start is None else t_start
    first, n_used = pref.pulse_ranges(c["n_pulses"], shift)
    pos, vel = np.asarray(c["pos"], dtype=np.float64), np.asarray(c["vel"], dtype=np.float64)
    t_p = np.asarray(c["t_vec"], dtype=np.float64)
    sl = slice(first[chan], first[chan] + n_used)
    v_hat = vel / np.linalg.norm(vel, axis=1, keepdims=True)
    p_tx = pos[sl][:, None, :]
    p_rx = p_tx + c["rx_offsets"][chan] * v_hat[sl][:, None, :]
    g = _grid(c)[None, :, :] + np.asarray(c["vel_focus"], dtype=np.float64).reshape(1, 1, 3) * (t_p - np.mean(t_p))[sl].reshape(-1, 1, 1)
    tau = (np.linalg.norm(g - p_tx, axis=2) + np.linalg.norm(g - p_rx, axis=2)) / k["C"]
    return (tau - t_start + c["chirp_centre"]) * k["FS"]


def all_idx_f(c, shift=False, t_start=None):
    """[idx_f] of every image of the case."""
    if c["kind"] == "pair":
        return [pair_idx_f(c, ch, shift, t_start) for ch in range(2)]
    return [focus_idx_f(c, t_start)]


def idx_norm_of(c, idx_f):
    """The normalised coordinate as each formula groups it: 2 (idx_f / n) - 1 in the focus, 2 idx_f / n - 1 in the pair."""
    n = c["num_samples"]
    return 2 * idx_f / n - 1 if c["kind"] == "pair" else 2 * (idx_f / n) - 1


def sample_position(idx_norm, n_s):
    """(x float32, i0 int64) of oracle.tdbp_oracle._grid_sample_1d: float32 coordinate, unnormalised with one rounding."""
    xn = np.asarray(idx_norm).astype(np.float32)
    x = ((xn + np.float32(1)).astype(np.float64) * (n_s / 2) - 0.5).astype(np.float32)
    return x, np.floor(x).astype(np.int64)


CLASSES = ("below", "lo_edge", "inside", "hi_edge", "above")


def index_census(c, shift=False, t_start=None):
    """(pulse, pixel) pairs per class of i0 over every image of the case - below: i0 < -1 (both taps padded), lo_edge: i0 == -1,
    inside: 0 <= i0 < n_s - 1, hi_edge: i0 == n_s - 1, above: i0 >= n_s - and the extremes of i0 and idx_f."""
    n = c["num_samples"]
    idx = all_idx_f(c, shift, t_start)
    i0 = np.concatenate([sample_position(idx_norm_of(c, i), n)[1].ravel() for i in idx])
    out = dict(below=int((i0 < -1).sum()), lo_edge=int((i0 == -1).sum()), inside=int(((i0 >= 0) & (i0 < n - 1)).sum()),
               hi_edge=int((i0 == n - 1).sum()), above=int((i0 >= n).sum()), i0_min=int(i0.min()), i0_max=int(i0.max()),
               idx_f_min=float(min(i.min() for i in idx)), idx_f_max=float(max(i.max() for i in idx)))
    assert sum(out[k] for k in CLASSES) == i0.size
    return out


# ---- the tolerance ---------------------------------------------------------------------------------------------------------------

_floors = {}


def pixel_floor(c, shift=False):
    """What legitimately separates a single-precision device from the oracle per pixel, measured on the oracle alone.
    coord: pixel_err between the oracle at t_start and at t_start -+ COORD_SHIFT / FS (the larger sign) - float32 roundings of the
           interpolation coordinate that flip under the coordinate error the tile form documents;
    rc:    pixel_err between the oracle on its own compressed pulses and on those plus independent complex Gaussian error of
           relative L2 exactly RC_REL_L2;
    tol:   MARGIN x the larger of the two (flips are discrete: the device's worst pixel may collect a few more than the shifted
           oracle's did).  Over the channels of a pair the larger figure holds.
    Returns dict(coord, rc, tol, cap)."""
    key = (c["name"], c["kind"], bool(shift), c["nx"], c["ny"])
    if key in _floors:
        return _floors[key]
    base = oracle_images(c, shift)
    d = COORD_SHIFT / c["k"]["FS"]
    coord = max(max(pixel_err(a, b) for a, b in zip(oracle_images(c, shift, t_start=c["t_start"] + s * d), base)) for s in (1.0, -1.0))
    rng = np.random.default_rng(SEED_FLOOR)
    noisy = []
    for r in (rc_of(c) if c["kind"] == "pair" else [rc_of(c)]):
        e = rng.standard_normal(r.shape) + 1j * rng.standard_normal(r.shape)
        noisy.append(r + e * (RC_REL_L2 * np.linalg.norm(r) / np.linalg.norm(e)))
    rc = max(pixel_err(a, b) for a, b in zip(oracle_images(c, shift, rc=noisy if c["kind"] == "pair" else noisy[0]), base))
    n_used = c["n_pulses"] - (1 if (shift and c["kind"] == "pair") else 0)
    _floors[key] = dict(coord=coord, rc=rc, tol=MARGIN * max(coord, rc), cap=cap(n_used))
    return _floors[key]
