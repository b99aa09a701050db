"""GMTI detection on the GPU (sarx.gmti_detect, focus_ati_dpca(detect=...), TwoChannelBatch(stack="detections")) against the NumPy
restatement of its semantics (tests/_gmti_numpy.py), on synthetic planes and on the C3 scene."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmti_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu

LAM, V, LAG = 0.031, 7500.0, 1.0 / 6000.0


def _synthetic(n_az, n_rg, seed):
    """Exponential clutter (P ~ Exp(1)), strong peaks up to 60 dB over it, equal-valued neighbours (ties) and a run of equal
    cells; complex images whose DPCA magnitude is NOT the plane (the plane is given explicitly)."""
    rng = np.random.default_rng(seed)
    m = np.sqrt(rng.exponential(1.0, (n_az, n_rg))).astype(np.float32)
    k = max(4, n_az * n_rg // 2000)
    ii, jj = rng.integers(0, n_az, k), rng.integers(0, n_rg, k)
    m[ii, jj] = np.sqrt(10.0 ** rng.uniform(1.5, 6.0, k)).astype(np.float32)
    for t in range(min(k, 40)):                                   # ties inside a guard box
        i, j = ii[t], jj[t]
        m[i, min(j + 1, n_rg - 1)] = m[i, j]
        if t % 3 == 0:
            m[min(i + 1, n_az - 1), max(j - 1, 0)] = m[i, j]
    m[n_az // 2, : min(n_rg, 9)] = 40.0                          # a run of equal cells at the left edge
    m[0, 0] = m[-1, -1] = 1e3                                     # corners: untested (too few training cells)
    s1 = (rng.standard_normal((n_az, n_rg)) + 1j * rng.standard_normal((n_az, n_rg))).astype(np.complex64)
    s2 = (s1 * np.exp(-0.3j) + 0.1 * (rng.standard_normal((n_az, n_rg)) + 1j * rng.standard_normal((n_az, n_rg)))).astype(np.complex64)
    return m, s1, s2


CASES = [((64, 64), (2, 2), (8, 8), 1e-3, 0.0),
         ((96, 80), (1, 3), (20, 6), 1e-3, 0.4),                  # HA = 32, HR = 16; n_rg not a multiple of the tile
         ((1000, 777), (2, 2), (8, 8), 1e-4, -1.1),
         ((1000, 777), (0, 4), (3, 28), 1e-4, 0.0),               # HA = 8, HR = 32
         ((4096, 4096), (2, 2), (8, 8), 1e-5, 0.0)]


def _assert_parity(m, s1, s2, guard, train, pfa, cal):
    import sarx
    n_az, n_rg = m.shape
    ra, ca = 5e5 + 0.25 * np.arange(n_rg), 1.2 * (np.arange(n_az) - n_az / 2)
    rep = sarx.gmti_detect(s1.T, s2.T, ra, ca, wavelength_m=LAM, platform_speed_mps=V, lag_s=LAG, guard=guard, train=train, pfa=pfa,
                           cal_phase=cal, max_detections=65536, dpca_mag=m.T)
    o = ref.cfar(m, guard, train, pfa=pfa)
    d = rep.detections
    cells = list(zip(d["i"].tolist(), d["j"].tolist()))
    assert cells == sorted(cells)                                 # sorted by (i, j)
    missing, extra = ref.compare(cells, o)
    assert not missing and not extra, (missing[:10], extra[:10], len(cells), len(o["cells"]))
    assert len(o["cells"]) > 3
    assert rep.alpha == pytest.approx(ref.cfar_alpha(pfa, ref.n_full(guard, train)), rel=1e-14)
    ii, jj = d["i"], d["j"]
    np.testing.assert_array_equal(d["power"], o["power"][ii, jj])
    np.testing.assert_allclose(d["mean"], o["mean"][ii, jj], rtol=1e-6)
    want = ref.interferogram(s1, s2, cells, cal)
    scale = np.array([np.sum(np.abs(s1[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2]) * np.abs(s2[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2]))
                      for i, j in cells])
    assert np.all(np.abs(d["interf"] - want) <= 1e-6 * scale)
    np.testing.assert_allclose(d["mag1"], np.abs(s1[ii, jj]), rtol=5e-7)
    np.testing.assert_allclose(d["mag2"], np.abs(s2[ii, jj]), rtol=5e-7)
    np.testing.assert_array_equal(d["range_m"], ra[jj])
    np.testing.assert_array_equal(d["cross_range_m"], ca[ii])
    np.testing.assert_allclose(d["v_los_mps"], -LAM * np.angle(want) / (4 * np.pi * LAG), atol=1e-4)
    np.testing.assert_allclose(d["cross_range_relocated_m"], ca[ii] + ra[jj] * d["v_los_mps"] / V, rtol=1e-12)
    assert rep.v_ambiguity_mps == pytest.approx(LAM / (4 * LAG))


@pytest.mark.parametrize("shape,guard,train,pfa,cal", CASES, ids=[f"{c[0][0]}x{c[0][1]}-g{c[1]}-t{c[2]}" for c in CASES])
def test_parity_on_synthetic_planes(shape, guard, train, pfa, cal):
    n_az, n_rg = shape
    _assert_parity(*_synthetic(n_az, n_rg, seed=n_az + 7 * n_rg + guard[1]), guard, train, pfa, cal)


LADDER = (8, 9, 16, 17)                   # outer half-widths at the steps of the halo ladder: HA, HR = 8, 16, 16, 32
LADDER_GUARD = (2, 2)


@functools.lru_cache(maxsize=None)
def _ladder_plane():
    planes = _synthetic(96, 80, seed=96 + 7 * 80)                 # past one tile in both directions
    for x in planes:
        x.setflags(write=False)
    return planes


@pytest.mark.parametrize("outer_rg", LADDER)
@pytest.mark.parametrize("outer_az", LADDER)
def test_parity_on_every_rung_of_the_halo_ladder(outer_az, outer_rg):
    """The sixteen windows reach all nine (HA, HR) instantiations of the CFAR kernel; _assert_parity holds every case to a
    non-empty reference list."""
    train = (outer_az - LADDER_GUARD[0], outer_rg - LADDER_GUARD[1])
    _assert_parity(*_ladder_plane(), LADDER_GUARD, train, 1e-3, 0.4)


def test_determinism_and_overflow():
    import sarx
    m, s1, s2 = _synthetic(1000, 777, seed=3)
    ra, ca = np.arange(777.0), np.arange(1000.0)
    kw = dict(wavelength_m=LAM, platform_speed_mps=V, lag_s=LAG, pfa=1e-3, dpca_mag=m.T)
    a = sarx.gmti_detect(s1.T, s2.T, ra, ca, **kw)
    b = sarx.gmti_detect(s1.T, s2.T, ra, ca, **kw)
    assert a.n_found > 100
    assert a.detections.tobytes() == b.detections.tobytes()
    with pytest.raises(sarx.GmtiOverflowError) as e:
        sarx.gmti_detect(s1.T, s2.T, ra, ca, max_detections=a.n_found - 1, **kw)
    assert str(a.n_found) in str(e.value) and e.value.count == a.n_found
    c = sarx.gmti_detect(s1.T, s2.T, ra, ca, max_detections=a.n_found, **kw)      # exactly full: no overflow
    assert c.detections.tobytes() == a.detections.tobytes()


def _peaks(img, k, half=8):
    """k strongest local peaks of |img|: argmax, then blank a (2 half + 1)^2 window, repeat."""
    a = np.abs(img).astype(np.float64).copy()
    out = []
    for _ in range(k):
        i, j = np.unravel_index(np.argmax(a), a.shape)
        out.append((int(i), int(j), float(a[i, j])))
        a[max(i - half, 0):i + half + 1, max(j - half, 0):j + half + 1] = 0
    return out


def test_c3_scene_movers_velocity_and_relocation(monkeypatch):
    """The C3 scene at n = 2048, scene_scale 0.25, both channels synthesised on the device over 2049 pulses with thermal noise of
    their own: the 15 m/s and 2 m/s movers are reported at their DPCA peaks, their radial speed is the geometry's, nothing is
    reported on the stationary grid, and the relocation puts each mover within 3 azimuth cells of where its stationary twin is
    imaged."""
    import sarx
    from sarx import radar
    from sarx.batch import TwoChannelBatch
    from sarx.engine import DeviceArray
    ctx = sarx.default_context()
    n = 2048
    params = sarx.GmtiParams(guard=(3, 16), train=(8, 8), pfa=1e-6, max_detections=4096)
    movers = [(g[0][0]["position"], g[1]) for g in radar.c3_scene(0)[1:]]        # [(p0, v)]: 15 m/s, 2 m/s

    def focus(noise, detect):
        b = TwoChannelBatch(ctx, n, 1, stack="multilook", scene="c3", scene_scale=0.25)
        b.prepare()
        rx = [DeviceArray(b._alloc[0][ch], (n + 1, n), owner=False) for ch in (0, 1)]
        if noise:
            p_mean = sarx.power_stats(b._alloc[0][0], (n + 1) * n)[1]
            for ch, seed in ((0, 11), (1, 12)):
                sarx.add_noise_dev(b._alloc[0][ch], (n + 1) * n, p_mean, 10.0, scr_db=None, seed=seed)
        res = sarx.focus_ati_dpca(rx[0], rx[1], *b.focus_args, detect=detect)
        k = b.k
        b.close()
        return res, k

    res, k = focus(True, params)
    orig = radar.c3_scene
    monkeypatch.setattr(radar, "c3_scene", lambda f=0, frame_dt=0.1: [(t, [0.0, 0.0, 0.0]) for t, _ in orig(f, frame_dt)])
    twin, _ = focus(False, None)
    monkeypatch.undo()

    d = res["detections"].detections
    cells = set(zip(d["i"].tolist(), d["j"].tolist()))
    ra, ca = res["range_axis"], res["cross_range"]
    dcr = ca[1] - ca[0]
    peaks = _peaks(twin["slc1"].T, 27)
    mover_px, grid_px = peaks[:2], peaks[2:]                                     # rcs 2000, 1500 against <= 340 on the grid
    dpca = res["dpca_mag"].T
    p_tx = radar.orbit_track(np.array([0.0]), k)[0][0]
    for (p0, vel), (ti, tj, _) in zip(movers, mover_px):
        pos = np.array([p0[0] * 0.25, p0[1] * 0.25, p0[2]])
        u = (pos - p_tx) / np.linalg.norm(pos - p_tx)
        v_true = float(np.dot(vel, u))
        win = dpca[:, max(tj - 25, 0):tj + 26]
        pi, pj = np.unravel_index(np.argmax(win), win.shape)
        pj += max(tj - 25, 0)
        assert (int(pi), int(pj)) in cells, (vel, (pi, pj), (ti, tj))
        r = d[(d["i"] == pi) & (d["j"] == pj)][0]
        assert abs(r["v_los_mps"] - v_true) < 0.5, (vel, r["v_los_mps"], v_true)
        assert abs(r["cross_range_relocated_m"] - ca[ti]) <= 3 * dcr, (vel, r["cross_range_relocated_m"], ca[ti], ca[pi])
    for gi, gj, _ in grid_px:
        near = [(i, j) for i, j in cells if abs(i - gi) <= 2 and abs(j - gj) <= 2]
        assert not near, ((gi, gj), near)
    assert res["detections"].v_ambiguity_mps == pytest.approx(k["Lambda"] * k["PRF"] / 4)


@pytest.mark.parametrize("n_az,n_rg", [(256, 256), (200, 240)])
def test_fused_equals_standalone(n_az, n_rg):
    import sarx
    from oracle import csa_oracle as orc
    (r1, r2), k = orc.point_scene(n_az, n_rg, seed=5, clutter_db=-25.0, two_channel=True)
    args = orc.focus_args(k)
    params = sarx.GmtiParams(pfa=1e-3, max_detections=8192)
    res = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, detect=params, cal_phase=0.2, return_slc2=False)
    full = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, cal_phase=0.2)
    alone = sarx.gmti_detect(full["slc1"], full["slc2"], full["range_axis"], full["cross_range"], wavelength_m=args[0],
                             platform_speed_mps=args[5], lag_s=1.0 / args[4], pfa=1e-3, cal_phase=0.2, max_detections=8192)
    a, b = res["detections"].detections, alone.detections
    assert len(a) > 3
    assert a.tobytes() == b.tobytes()
    dev = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, detect=params, cal_phase=0.2, device_output=True)
    assert dev["detections"].detections.tobytes() == a.tobytes()
    for key in ("slc1", "slc2", "slc1_mag", "dpca_mag", "ati_phase_masked"):
        if key in dev:
            dev[key].release()


def test_batch_detections_match_the_reference_on_the_product_planes():
    import sarx
    from sarx.batch import TwoChannelBatch
    ctx = sarx.default_context()
    n, frames = 1024, 3
    p = sarx.GmtiParams(max_detections=65536)
    b = TwoChannelBatch(ctx, n, frames, stack="detections", scene="c3", scene_scale=0.25, detect=p)
    assert b.slot_bytes == 16 + 48 * 65536
    b.run()
    ctx.sync()
    reports = [b.detections(f) for f in range(frames)]
    b.close()
    bp = TwoChannelBatch(ctx, n, frames, stack="products", scene="c3", scene_scale=0.25)
    bp.run()
    ctx.sync()
    st = bp.stack()
    bp.close()
    for f in range(frames):
        o = ref.cfar(st[f, 2], p.guard, p.train, pfa=p.pfa)
        cells = list(zip(reports[f].detections["i"].tolist(), reports[f].detections["j"].tolist()))
        missing, extra = ref.compare(cells, o)
        assert not missing and not extra, (f, missing[:10], extra[:10])
        assert 1 <= reports[f].n_found < p.max_detections, reports[f].n_found
        print(f"frame {f}: {reports[f].n_found} reports")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_ranks_one_gpu_detection_stack_equals_single_rank(tmp_path):
    import sarx
    from sarx.batch import TwoChannelBatch
    n, frames, max_det = 512, 3, 16384
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "_gmti_batch_worker.py"), str(tmp_path), str(n),
           str(frames), str(max_det)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    s0 = np.load(tmp_path / "gmti_stack_rank0.npy")
    s1 = np.load(tmp_path / "gmti_stack_rank1.npy")
    assert s0.tobytes() == s1.tobytes()
    ctx = sarx.default_context()
    b = TwoChannelBatch(ctx, n, frames, stack="detections", scene="c3", scene_scale=0.25, detect=sarx.GmtiParams(max_detections=max_det))
    b.run()
    ctx.sync()
    single = b.stack()
    assert s0[:frames].tobytes() == single.tobytes()
    assert (s0[frames:] == 0).all()
    assert all(b.detections(f).n_found >= 1 for f in range(frames))
    b.close()
