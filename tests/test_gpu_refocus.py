"""GMTI refocus on the GPU (sarx.gmti_refocus, focus_ati_dpca(refocus=...), TwoChannelBatch(refocus=...)) against the NumPy
restatement of its semantics (tests/_refocus_numpy.py), on synthetic images and on the C3 scene."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _refocus_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# an airborne geometry in which a few m/s along track is a visible smear over a 64 .. 512-pulse chip
LAM, V, PRF, R0, DR = 0.031, 200.0, 1000.0, 5000.0, 1.0


def _params(L, W, source="dpca", **kw):
    import sarx
    return sarx.RefocusParams(chip=(L, W), v_along=(-30.0, 30.0), n_hyp=13, source=source, want_curves=True, want_chips=True, **kw)


def _scene(n_az, n_rg, seed, cal, positions, L, W, speeds):
    """Clutter common to both channels (cancelled by the DPCA difference up to a little noise), and at every position a point
    in slc1 smeared by the inverse of a known hypothesis."""
    rng = np.random.default_rng(seed)
    clutter = (0.3 * (rng.standard_normal((n_az, n_rg)) + 1j * rng.standard_normal((n_az, n_rg))))
    s1 = clutter.copy()
    s2 = clutter * np.exp(-1j * cal) + 0.02 * (rng.standard_normal((n_az, n_rg)) + 1j * rng.standard_normal((n_az, n_rg)))
    truth = []
    for q, (i, j) in enumerate(positions):
        k = (3 * q + 2) % len(speeds)
        d = np.zeros((n_az, n_rg), np.complex128)
        d[i, j] = 20.0 * np.exp(0.7j * q)
        ref.smear(d, i, j, L, W, LAM, V, PRF, R0, DR, speeds[k])
        s1 += d
        truth.append(k)
    return s1.astype(np.complex64), s2.astype(np.complex64), truth


def _axes(n_az, n_rg):
    return R0 + DR * np.arange(n_rg), np.arange(n_az, dtype=np.float64)


def _check_against_reference(res, s1, s2, positions, L, W, speeds, source, cal):
    want = ref.refocus(s1, s2, positions, L, W, speeds, LAM, V, PRF, R0, DR, source, cal)
    assert len(res) == len(want)
    for q, w in enumerate(want):
        np.testing.assert_allclose(res.curves[q], w["curve"], rtol=1e-4, err_msg=f"report {q}")
        top = np.sort(w["curve"])[::-1]
        r = res.records[q]
        assert r["i0"] == w["i0"]
        assert r["sharpness_identity"] == pytest.approx(w["s_identity"], rel=1e-4)
        if len(top) > 1 and top[0] - top[1] <= 1e-4 * top[0]:
            continue                                            # k* not defined at fp32 resolution
        assert r["k_best"] == w["k_best"], (q, r["k_best"], w["k_best"])
        y = res.chips[q].astype(np.complex128)
        assert np.linalg.norm(y - w["chip"]) <= 1e-5 * np.linalg.norm(w["chip"]), q
        assert (r["peak_i"], r["peak_j"]) == (w["peak_i"], w["peak_j"]), q
        assert r["sharpness"] == pytest.approx(w["s_best"], rel=1e-4)
        assert 10 ** (r["refocus_gain_db"] / 10) == pytest.approx(w["peak_power"] / w["orig_power"], rel=1e-4)


CASES = [(64, 1, "dpca", 0.7), (64, 15, "slc1", 0.0), (256, 5, "dpca", -1.2), (256, 15, "dpca", 0.3), (128, 9, "dpca", 0.0),
         (512, 1, "slc1", 0.0), (512, 5, "dpca", 2.0), (512, 15, "dpca", 0.4)]


@pytest.mark.parametrize("L,W,source,cal", CASES, ids=[f"L{c[0]}-W{c[1]}-{c[2]}" for c in CASES])
def test_parity_on_synthetic_images(L, W, source, cal):
    import sarx
    n_az, n_rg = 700, 203                                     # n_rg odd, prime to every tile size
    positions = np.array([(3, 100), (n_az - 2, 60), (350, 0), (200, n_rg - 1), (500, 30), (420, 140)], np.int64)
    p = _params(L, W, source)
    speeds = p.speeds(V)
    s1, s2, truth = _scene(n_az, n_rg, 7 + L + W, cal, positions, L, W, speeds)
    ra, ca = _axes(n_az, n_rg)
    res = sarx.gmti_refocus(positions, s1.T, s2.T, ra, ca, wavelength_m=LAM, platform_speed_mps=V, prf_hz=PRF, params=p, cal_phase=cal)
    _check_against_reference(res, s1, s2, positions, L, W, speeds, source, cal)
    # each smeared point is found at its own hypothesis and comes back a point (where the grid step is a visible phase)
    for q, k in enumerate(truth if source == "dpca" and L >= 128 else []):
        assert res.records[q]["k_best"] == k, (q, res.records[q]["k_best"], k)
        assert (res.records[q]["peak_i"], res.records[q]["peak_j"]) == tuple(positions[q])
    # the same call without curves and chips gives the same records
    p2 = _params(L, W, source)
    p2.want_curves = p2.want_chips = False
    res2 = sarx.gmti_refocus(positions, s1.T, s2.T, ra, ca, wavelength_m=LAM, platform_speed_mps=V, prf_hz=PRF, params=p2, cal_phase=cal)
    assert res2.curves is None and res2.chips is None
    assert res2.records.tobytes() == res.records.tobytes()


def test_slc1_source_without_slc2_and_determinism():
    import sarx
    n_az, n_rg = 600, 77
    positions = np.array([(300, 40), (10, 5), (590, 76)], np.int64)
    p = _params(256, 5, "slc1")
    s1, s2, _ = _scene(n_az, n_rg, 3, 0.0, positions, 256, 5, p.speeds(V))
    ra, ca = _axes(n_az, n_rg)
    kw = dict(wavelength_m=LAM, platform_speed_mps=V, prf_hz=PRF, params=p)
    a = sarx.gmti_refocus(positions, s1.T, None, ra, ca, **kw)
    b = sarx.gmti_refocus(positions, s1.T, None, ra, ca, **kw)
    _check_against_reference(a, s1, None, positions, 256, 5, p.speeds(V), "slc1", 0.0)
    assert a.records.tobytes() == b.records.tobytes()
    assert a.curves.tobytes() == b.curves.tobytes() and a.chips.tobytes() == b.chips.tobytes()
    pd = _params(256, 5, "dpca")
    with pytest.raises(ValueError):
        sarx.gmti_refocus(positions, s1.T, None, ra, ca, wavelength_m=LAM, platform_speed_mps=V, prf_hz=PRF, params=pd)


def _raw_call(ctx, s1, s2, header, n_rep, max_det, p):
    """sarx_refocus_dev on a hand-made slot; returns the record, curve and chip bytes (pre-filled with 0xAB)."""
    from sarx import gmti, refocus
    n_az, n_rg = s1.shape
    slot = np.zeros(gmti.HEADER_BYTES + max_det * gmti.REPORT_DTYPE.itemsize, np.uint8)
    slot[:16].view("<u4")[:] = header
    rep = slot[16:].view(gmti.REPORT_DTYPE)
    rep["i"][:n_rep], rep["j"][:n_rep] = n_az // 2, n_rg // 2
    L, W = p.validate()
    fill = {k: np.full(nb, 0xAB, np.uint8) for k, nb in (("rec", max_det * 48), ("curves", max_det * p.n_hyp * 4),
                                                          ("chips", max_det * L * W * 8))}
    bufs = {k: ctx.to_device(v) for k, v in fill.items()}
    d1, d2, ds = ctx.to_device(s1), ctx.to_device(s2), ctx.to_device(slot)
    try:
        cp = p.c_params(LAM, V, PRF, R0, DR, 0.0)
        refocus.enqueue(ctx, d1.ptr, d2.ptr, n_az, n_rg, cp, ds.ptr, max_det, bufs["rec"].ptr, bufs["curves"].ptr, bufs["chips"].ptr)
        return {k: bufs[k].download(np.uint8, (len(fill[k]),)).copy() for k in fill}
    finally:
        for b in (d1, d2, ds, *bufs.values()):
            b.release()


def test_empty_list_and_overflowed_slot_write_nothing():
    import sarx
    from sarx import refocus
    ctx = sarx.default_context()
    n_az, n_rg = 256, 40
    s1, s2, _ = _scene(n_az, n_rg, 1, 0.0, [], 64, 5, [V])
    p = _params(64, 5)
    out = _raw_call(ctx, s1, s2, [0, 0, 0, 0], 0, 8, p)                   # count 0
    assert all((v == 0xAB).all() for v in out.values())
    out = _raw_call(ctx, s1, s2, [9, 1, 0, 0], 8, 8, p)                   # 9 qualifying cells, capacity 8: overflow
    assert all((v == 0xAB).all() for v in out.values())
    out = _raw_call(ctx, s1, s2, [3, 0, 0, 0], 8, 8, p)                   # three reports: records 0..2 written, 3.. untouched
    assert not (out["rec"][:3 * 48] == 0xAB).all() and (out["rec"][3 * 48:] == 0xAB).all()
    res = sarx.gmti_refocus(np.zeros((0, 2), np.int64), s1.T, s2.T, *_axes(n_az, n_rg), wavelength_m=LAM, platform_speed_mps=V,
                            prf_hz=PRF, params=p)
    assert len(res) == 0 and res.curves.shape == (0, p.n_hyp)
    # the host side of an overflowed slot
    slot = np.zeros(16 + 8 * 48, np.uint8)
    slot[:8].view("<u4")[:] = [9, 1]
    d1, d2, ds = ctx.to_device(s1), ctx.to_device(s2), ctx.to_device(slot)
    try:
        with pytest.raises(sarx.GmtiOverflowError):
            refocus.refocus_slot(ctx, d1.ptr, d2.ptr, n_az, n_rg, p, _axes(n_az, n_rg)[0], ds.ptr, 8, wavelength_m=LAM,
                                 platform_speed_mps=V, prf_hz=PRF)
    finally:
        for b in (d1, d2, ds):
            b.release()


def test_fused_equals_standalone():
    import sarx
    from oracle import csa_oracle as orc
    (r1, r2), k = orc.point_scene(256, 256, seed=5, clutter_db=-25.0, two_channel=True)
    args = orc.focus_args(k)
    det = sarx.GmtiParams(pfa=1e-3, max_detections=8192)
    rp = sarx.RefocusParams(chip=(64, 5), want_curves=True, footprint_speed_mps=args[5] * 0.97)
    res = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, detect=det, refocus=rp, cal_phase=0.2)
    alone = sarx.gmti_refocus(res["detections"], res["slc1"], res["slc2"], res["range_axis"], res["cross_range"],
                              wavelength_m=args[0], platform_speed_mps=args[5], prf_hz=args[4], params=rp, cal_phase=0.2)
    a = res["refocus"]
    assert len(a) == len(res["detections"]) > 3
    assert a.records.tobytes() == alone.records.tobytes()
    assert a.curves.tobytes() == alone.curves.tobytes()
    np.testing.assert_array_equal(a["i"], res["detections"].detections["i"])
    with pytest.raises(ValueError):
        sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, refocus=rp)


def test_batch_refocus_equals_standalone():
    import sarx
    from sarx import radar
    from sarx.batch import TwoChannelBatch
    ctx = sarx.default_context()
    n = 1024
    det = sarx.GmtiParams(max_detections=4096)
    b = TwoChannelBatch(ctx, n, 1, stack="detections", scene="c3", scene_scale=0.25, detect=det,
                        refocus=sarx.RefocusParams(chip=(128, 5)))
    assert b.slot_bytes == 16 + 48 * 4096 + 48 * 4096
    b.run()
    ctx.sync()
    rep = b.detections(0)
    got = b.refocus(0)
    kc = b.k
    vg = kc["V_sat"] * kc["Re"] / kc["R_sat"]
    ra, ca = b.plan.axes()
    alone = sarx.gmti_refocus(rep, b.s1, b.s2, ra, ca, wavelength_m=kc["Lambda"], platform_speed_mps=kc["V_eff"], prf_hz=kc["PRF"],
                              params=sarx.RefocusParams(chip=(128, 5), footprint_speed_mps=vg), ctx=ctx)
    b.close()
    assert len(got) == rep.n_found >= 1
    assert got.records.tobytes() == alone.records.tobytes()
    plain = TwoChannelBatch(ctx, n, 1, stack="detections", scene="c3", scene_scale=0.25, detect=det)
    assert plain.slot_bytes == det.slot_bytes()                 # no refocus: the slot is what it was
    plain.close()
    assert radar.reference_constants()["V_sat"] > vg


def test_c3_scene_along_track_mover_is_measured_and_refocused(monkeypatch):
    """The C3 scene of test_gpu_gmti.py (n = 2048, scene_scale 0.25, thermal noise) with the 15 m/s mover given a 30 m/s
    along-track component.  Over 2049 pulses (0.34 s) that is about 5.3 rad of quadratic phase at the aperture edge, 17 samples
    of smear and a peak loss of roughly 6 dB: the search must find v_along within 15 % of 30 m/s with the right sign and gain at
    least 3 dB.  The 2 m/s radial mover of the same scene, and the purely radial 15 m/s mover of the unmodified scene, stay where
    they are (|v_along| <= 4.5 m/s, gain < 1 dB)."""
    import sarx
    from sarx import radar
    from sarx.batch import TwoChannelBatch
    from sarx.engine import DeviceArray
    ctx = sarx.default_context()
    n = 2048
    det = sarx.GmtiParams(guard=(3, 16), train=(8, 8), pfa=1e-6, max_detections=4096)
    orig = radar.c3_scene

    def focus():
        b = TwoChannelBatch(ctx, n, 1, stack="multilook", scene="c3", scene_scale=0.25)
        b.prepare()
        rx = [DeviceArray(b._alloc[0][ch], (n + 1, n), owner=False) for ch in (0, 1)]
        p_mean = sarx.power_stats(b._alloc[0][0], (n + 1) * n)[1]
        for ch, seed in ((0, 11), (1, 12)):
            sarx.add_noise_dev(b._alloc[0][ch], (n + 1) * n, p_mean, 10.0, scr_db=None, seed=seed)
        k = b.k
        vg = k["V_sat"] * k["Re"] / k["R_sat"]
        rp = sarx.RefocusParams(chip=(128, 5), footprint_speed_mps=vg, want_curves=True)
        res = sarx.focus_ati_dpca(rx[0], rx[1], *b.focus_args, detect=det, refocus=rp)
        b.close()
        return res, k

    def mover(res, k, p0, vel):
        """The strongest report whose ATI radial speed is the mover's."""
        p_tx = radar.orbit_track(np.array([0.0]), k)[0][0]
        pos = np.array([p0[0] * 0.25, p0[1] * 0.25, p0[2]])
        u = (pos - p_tx) / np.linalg.norm(pos - p_tx)
        v_los = float(np.dot(vel, u))
        d = res["detections"].detections
        sel = np.flatnonzero(np.abs(d["v_los_mps"] - v_los) < max(0.3 * abs(v_los), 0.5))
        assert len(sel), (vel, v_los)
        q = sel[np.argmax(d["power"][sel])]
        return res["refocus"].records[q]

    movers = [(g[0][0]["position"], g[1]) for g in orig(0)[1:]]            # 15 m/s, 2 m/s radial
    monkeypatch.setattr(radar, "c3_scene", lambda f=0, frame_dt=0.1: [(t, [15.0, 30.0, 0.0]) if q == 1 else (t, v)
                                                                      for q, (t, v) in enumerate(orig(f, frame_dt))])
    res, k = focus()
    monkeypatch.undo()
    fast = mover(res, k, movers[0][0], [15.0, 30.0, 0.0])
    slow = mover(res, k, movers[1][0], movers[1][1])
    plain, _ = focus()
    radial = mover(plain, k, movers[0][0], movers[0][1])
    print("along-track mover", fast, "\nslow mover", slow, "\nradial mover", radial)
    assert abs(fast["v_along_mps"] - 30.0) <= 0.15 * 30.0, fast
    assert fast["refocus_gain_db"] >= 3.0, fast
    for r in (slow, radial):
        assert abs(r["v_along_mps"]) <= 4.5, r
        assert r["refocus_gain_db"] < 1.0, r
