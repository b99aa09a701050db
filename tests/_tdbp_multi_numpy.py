"""fp64 NumPy restatement of the N-receiver back-projection and the multi-baseline ATI resolver (include/sarx_tdbp_multi.h).
TEST INFRASTRUCTURE ONLY.

The images are the pair's restatement (tests/_tdbp_pair_numpy.pair_images) called on the channels (0, c); the resolver is written
from the header.  It also fixes the scenes that tests/test_tdbp_multi.py (physics, CPU) and tests/test_gpu_tdbp_multi.py (parity,
GPU) share: the scaled radar, six stationary scatterers, one mover, receivers at multiples of d = V / PRF along track."""
import functools

import numpy as np

from oracle import csa_oracle as co
from oracle import tdbp_oracle as tb

import _tdbp_pair_numpy as pref

rel_l2 = pref.rel_l2
RECORD_DTYPE = np.dtype([("v_los", "<f8"), ("v_coarse", "<f8"), ("cost", "<f8"), ("cost_next", "<f8"), ("phase", "<f8", (3,)),
                         ("k", "<i4"), ("status", "<u4")])


def scene(n_pulses, k, stationary, movers, offsets_d):
    """An n_rx-receiver CPI on the VideoSAR arc: receiver c at offsets_d[c] * V / PRF along track, echoes of
    oracle.csa_oracle.echo_bistatic on the exact 1 / FS grid over the spotlight window, cast to complex64.
    stationary: [(x, y, rcs)]; movers: [(x, y, rcs, (vx, vy, vz))], positions at t = 0."""
    n_s, t_start, _ = tb.spotlight_window(k)
    t_vec = (np.arange(n_pulses) - n_pulses / 2) / k["PRF"]
    pos, vel = tb.orbit_arc(t_vec, k)
    speed = float(np.linalg.norm(vel[n_pulses // 2]))
    offs = tuple(float(m) * speed / k["PRF"] for m in offsets_d)
    groups = [([(x, y, rcs) for x, y, rcs in stationary], np.zeros(3))] + [([(x, y, rcs)], np.asarray(v, float)) for x, y, rcs, v in movers]
    raw = []
    for off in offs:
        r = np.zeros((n_pulses, n_s), dtype=np.complex128)
        for tg, v in groups:
            if tg:
                r += co.echo_bistatic([{"position": [x, y, 0.0], "rcs": rcs} for x, y, rcs in tg], t_vec, pos, vel, off, v, n_s, k["FS"],
                                      t_start, k["FC"], k["K_RATE"], k["T_P"], linspace_grid=False)
        raw.append(r.astype(np.complex64))
    lags = tuple((o - offs[0]) / (2 * speed) for o in offs[1:])
    return dict(raw=raw, pos=pos, vel=vel, t_vec=t_vec, t_start=t_start, num_samples=n_s, k=k, rx_offsets=offs, speed=speed,
                chirp_centre=k["T_P"] / 2, lags=lags, wavelength=k["C"] / k["FC"], movers=list(movers))


def stack_images(sc, scene_size, nx, ny, first, n_used, vel_focus=(0.0, 0.0, 0.0), channels=None):
    """complex128 [n_rx x ny x nx]: pair_images on the channels (0, c); the channel-0 images of the calls must be the same bits.
    channels: which of the scene's channels make the stack (default all); the compression is done once per scene and kept on it."""
    if "rc" not in sc:
        sc["rc"] = [tb.range_compress(r, sc["num_samples"], sc["k"]) for r in sc["raw"]]
    ch = list(range(len(sc["raw"]))) if channels is None else list(channels)
    out = np.empty((len(ch), ny, nx), dtype=np.complex128)
    for n, c in enumerate(ch[1:], start=1):
        two = pref.pair_images([sc["raw"][ch[0]], sc["raw"][c]], sc["pos"], sc["vel"], sc["t_vec"], sc["t_start"], sc["num_samples"], scene_size,
                               nx, ny, sc["k"], (sc["rx_offsets"][ch[0]], sc["rx_offsets"][c]), sc["chirp_centre"], (first[0], first[n]), n_used,
                               vel_focus, rc=[sc["rc"][ch[0]], sc["rc"][c]])
        if n == 1:
            out[0] = two[0]
        assert two[0].tobytes() == out[0].tobytes()
        out[n] = two[1]
    return out


def wrap(x):
    """onto (-pi, pi]"""
    return x - 2 * np.pi * np.ceil((x - np.pi) / (2 * np.pi))


def resolve(imgs, cells, lags, wavelength, v_max, half=1):
    """The records of include/sarx_tdbp_multi.h, part 2, for the reports at `cells` [(i, j)] of the stack imgs [n_rx x ny x nx]
    (cast to complex64 first: the device reads that form)."""
    z = np.asarray(imgs).astype(np.complex64)
    n_rx, ny, nx = z.shape
    nb = n_rx - 1
    lags = [float(x) for x in lags]
    assert len(lags) == nb
    B = max(range(nb), key=lambda b: (abs(lags[b]), -b))
    S = min(range(nb), key=lambda b: (abs(lags[b]), b))
    lam = float(wavelength)
    out = np.zeros(len(cells), RECORD_DTYPE)
    for r, (i, j) in enumerate(cells):
        i0, i1, j0, j1 = max(i - half, 0), min(i + half, ny - 1), max(j - half, 0), min(j + half, nx - 1)
        w = np.zeros(nb, np.complex128)
        for ii in range(i0, i1 + 1):
            for jj in range(j0, j1 + 1):
                a = z[0, ii, jj]
                for b in range(nb):
                    c = z[b + 1, ii, jj]
                    w[b] += complex(float(a.real) * float(c.real) + float(a.imag) * float(c.imag),
                                    float(a.imag) * float(c.real) - float(a.real) * float(c.imag))
        phi = np.arctan2(w.imag, w.real)
        out["phase"][r, :nb] = phi
        if np.any(w == 0):
            out["status"][r] = 2
            continue
        out["v_coarse"][r] = -lam * phi[S] / (4 * np.pi * lags[S])
        best = None
        costs = []
        for k in range(-200, 201):
            v = -lam * (phi[B] + 2 * np.pi * k) / (4 * np.pi * lags[B])
            if not abs(v) <= v_max:
                continue
            cost = 0.0
            for b in range(nb):
                if b != B:
                    cost += float(wrap(phi[b] + 4 * np.pi * lags[b] * v / lam)) ** 2
            costs.append((cost, abs(k), 0 if k >= 0 else 1, k, v))
        if not costs:
            out["status"][r] = 1
            out["cost"][r] = out["cost_next"][r] = np.inf
            continue
        costs.sort()
        best = costs[0]
        out["v_los"][r], out["k"][r], out["cost"][r] = best[4], best[3], best[0]
        out["cost_next"][r] = costs[1][0] if len(costs) > 1 else np.inf
    return out


# the scene of the issue: receivers at (-d, +d, -d + 10 d), lags 1 / PRF and 5 / PRF; aligned pulse ranges (5, 4, 0), 315 used
OFFSETS_3 = (-1.0, 1.0, 9.0)
FIRST_3, N_USED = (5, 4, 0), 315
# a fourth receiver whose lag is no whole pulse: -d + 7.3 d; its range is set by hand, next to the aligned one (3.65 pulses: 1)
OFFSETS_4 = (-1.0, 1.0, 9.0, 6.3)
FIRST_4 = (5, 4, 0, 1)
GRID = (360.0, 90, 70)                # scene size, nx, ny


def mover_of(vy):
    return (49.5 * vy, 0.0, 50.0, (0.0, float(vy), 0.0))


@functools.lru_cache(maxsize=None)
def three_rx_scene(vy):
    """320 pulses of the scaled radar, the six scatterers of the pair's scenes and one mover of rcs 50 at (49.5 vy, 0) m with
    velocity (0, vy, 0): its radial speed brings it to the middle of the chip."""
    return scene(320, tb.scaled_constants(), pref.six_scatterers(), [mover_of(vy)], OFFSETS_3)


@functools.lru_cache(maxsize=None)
def four_rx_scene():
    """160 pulses, the six scatterers and a mover inside the chip; the fourth channel's lag is 3.65 pulses."""
    return scene(160, tb.scaled_constants(), pref.six_scatterers(), [(40.0, -30.0, 100.0, (0.0, 10.0, 0.0))], OFFSETS_4)


@functools.lru_cache(maxsize=None)
def three_rx_images(vy):
    return stack_images(three_rx_scene(vy), GRID[0], GRID[1], GRID[2], FIRST_3, N_USED)


def v_los_true(sc, vy):
    return pref.v_los_true(sc, (49.5 * vy, 0.0), (0.0, float(vy), 0.0))
