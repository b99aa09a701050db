"""fp64 NumPy restatement of the two-receiver back-projection (include/sarx_tdbp_pair.h).  TEST INFRASTRUCTURE ONLY.

Written from the header's semantics with the oracle's own pieces: oracle.tdbp_oracle.range_compress and _grid_sample_1d (the
float32 interpolation of F.grid_sample), echoes from oracle.csa_oracle.echo_bistatic.  It also fixes the scenes that
tests/test_tdbp_pair.py (physics, CPU) and tests/test_gpu_tdbp_pair.py (parity, GPU) share."""
import functools

import numpy as np

from oracle import csa_oracle as co
from oracle import tdbp_oracle as tb


def pulse_ranges(n_pulses, shift):
    """(first [2], n_used) of a pulse_shift flag."""
    return ((1, 0), n_pulses - 1) if shift else ((0, 0), n_pulses)


def pair_images(raw, pos_tx, vel_tx, t_pulses, t_start, num_samples, scene_size, nx, ny, k, rx_offsets, chirp_centre, first, n_used,
                vel_focus=(0.0, 0.0, 0.0), rc=None, batch=2048):
    """complex128 [2 x ny x nx].  raw: the two channels [n_pulses x num_samples] (complex64 as the device gets them); rc: their
    range-compressed form if the caller has it."""
    C, FC, FS = k["C"], k["FC"], k["FS"]
    pos = np.asarray(pos_tx, dtype=np.float64)
    vel = np.asarray(vel_tx, dtype=np.float64)
    t_p = np.asarray(t_pulses, dtype=np.float64)
    dt_all = t_p - np.mean(t_p)                                       # over ALL pulses: one definition for both channels
    v_hat = vel / np.linalg.norm(vel, axis=1, keepdims=True)
    v_f = np.asarray(vel_focus, dtype=np.float64).reshape(1, 1, 3)
    gx, gy = np.meshgrid(np.linspace(-scene_size / 2, scene_size / 2, nx), np.linspace(-scene_size / 2, scene_size / 2, ny), indexing="xy")
    grid = np.stack((gx.ravel(), gy.ravel(), np.zeros(gx.size)), axis=1)
    out = np.zeros((2, grid.shape[0]), dtype=np.complex128)
    for c in range(2):
        rcc = tb.range_compress(raw[c], num_samples, k) if rc is None else rc[c]
        sl = slice(first[c], first[c] + n_used)
        re32 = np.ascontiguousarray(rcc.real.astype(np.float32)[sl])
        im32 = np.ascontiguousarray(rcc.imag.astype(np.float32)[sl])
        p_tx = pos[sl][:, None, :]
        p_rx = p_tx + rx_offsets[c] * v_hat[sl][:, None, :]
        dt = dt_all[sl].reshape(-1, 1, 1)
        for b0 in range(0, grid.shape[0], batch):
            g = grid[None, b0:b0 + batch, :] + v_f * dt
            tau = (np.linalg.norm(g - p_tx, axis=2) + np.linalg.norm(g - p_rx, axis=2)) / C
            idx_f = (tau - t_start + chirp_centre) * FS
            idx_norm = 2 * idx_f / num_samples - 1
            s = tb._grid_sample_1d(re32, idx_norm).astype(np.float64) + 1j * tb._grid_sample_1d(im32, idx_norm).astype(np.float64)
            out[c, b0:b0 + batch] = np.sum(s * np.exp(1j * (2 * np.pi * FC * tau)), axis=0)
    return out.reshape(2, ny, nx)


def scene(n_pulses, k, stationary, movers=(), orbit="batch"):
    """A two-receiver CPI: receivers at -+ V / PRF along track (the DPCA condition: one pulse interval between the phase
    centres), echoes of oracle.csa_oracle.echo_bistatic on the exact 1 / FS grid over the spotlight window, cast to complex64.
    stationary: [(x, y, rcs)]; movers: [(x, y, rcs, (vx, vy, vz))], positions at t = 0.  orbit "batch": the VideoSAR arc (along
    track = x); "csa": the CSA script's track (along track = y = image rows)."""
    n_s, t_start, _ = tb.spotlight_window(k)
    t_vec = (np.arange(n_pulses) - n_pulses / 2) / k["PRF"]
    if orbit == "batch":
        pos, vel = tb.orbit_arc(t_vec, k)
    else:
        kc = co.reference_radar_constants()
        pos, vel = co.orbit_track(t_vec, kc)
    speed = float(np.linalg.norm(vel[n_pulses // 2]))
    offs = (-speed / k["PRF"], speed / k["PRF"])
    raw = []
    for off in offs:
        r = np.zeros((n_pulses, n_s), dtype=np.complex128)
        groups = [([(x, y, rcs) for x, y, rcs in stationary], np.zeros(3))] + [([(x, y, rcs)], np.asarray(v, float)) for x, y, rcs, v in movers]
        for tg, v in groups:
            if tg:
                r += co.echo_bistatic([{"position": [x, y, 0.0], "rcs": rcs} for x, y, rcs in tg], t_vec, pos, vel, off, v, n_s, k["FS"],
                                      t_start, k["FC"], k["K_RATE"], k["T_P"], linspace_grid=False)
        raw.append(r.astype(np.complex64))
    return dict(raw=raw, pos=pos, vel=vel, t_vec=t_vec, t_start=t_start, num_samples=n_s, k=k, rx_offsets=offs, speed=speed,
                chirp_centre=k["T_P"] / 2, lag=(offs[1] - offs[0]) / (2 * speed), movers=list(movers))


def images(sc, scene_size, nx, ny, shift, vel_focus=(0.0, 0.0, 0.0)):
    """pair_images of a scene dict; the compression is done once per scene and kept on it."""
    if "rc" not in sc:
        sc["rc"] = [tb.range_compress(r, sc["num_samples"], sc["k"]) for r in sc["raw"]]
    first, n_used = pulse_ranges(len(sc["t_vec"]), shift)
    return pair_images(sc["raw"], sc["pos"], sc["vel"], sc["t_vec"], sc["t_start"], sc["num_samples"], scene_size, nx, ny, sc["k"],
                       sc["rx_offsets"], sc["chirp_centre"], first, n_used, vel_focus, rc=sc["rc"])


def six_scatterers(seed=11, half=120.0):
    rng = np.random.default_rng(seed)
    return [(float(rng.uniform(-half, half)), float(rng.uniform(-half, half)), float(rng.uniform(1.0, 50.0))) for _ in range(6)]


MOVER_V = (0.0, 10.0, 0.0)            # ground range on the batch orbit: v_los = 10 sin(incidence)
MOVER_AT = (495.0, 0.0)               # the azimuth shift of its radial speed brings it to the middle of the chip
FOCUS_AT = (40.0, -30.0)              # the mover of the focus scene: inside the chip, imaged with vel_focus = its velocity


@functools.lru_cache(maxsize=None)
def stationary_scene():
    """Six stationary scatterers, 160 pulses of the scaled radar; imaged 40 x 40 over 400 m."""
    return scene(160, tb.scaled_constants(), six_scatterers())


@functools.lru_cache(maxsize=None)
def mover_scene():
    """The same scatterers and a mover at (495, 0) m with velocity (0, 10, 0) m/s, 320 pulses; imaged 90 x 70 over 360 m."""
    return scene(320, tb.scaled_constants(), six_scatterers(), [(MOVER_AT[0], MOVER_AT[1], 50.0, MOVER_V)])


@functools.lru_cache(maxsize=None)
def focus_scene():
    """The same scatterers and a stronger mover inside the chip, 320 pulses; imaged 40 x 40 over 400 m with vel_focus = its
    velocity."""
    return scene(320, tb.scaled_constants(), six_scatterers(), [(FOCUS_AT[0], FOCUS_AT[1], 400.0, MOVER_V)])


def v_los_true(sc, at, v):
    """Line-of-sight speed (positive = range opening) of velocity v at ground point `at` seen from mid-aperture."""
    p = sc["pos"][len(sc["t_vec"]) // 2]
    los = np.array([at[0], at[1], 0.0]) - p
    return float(np.dot(np.asarray(v, float), los / np.linalg.norm(los)))


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))
