"""Two-channel balance on the GPU (sarx.channel_balance, focus_ati_dpca(balance=...), include/sarx_balance.h) against the NumPy
restatement of its semantics (tests/_balance_numpy.py).

Bars.  Block sums: the fp64 products of fp32 samples are exact, so the GPU and the restatement differ by the order of the fp64
additions alone: 1e-12 of the sum of the terms' magnitudes (at most sqrt(S11 S22) for S12) is four orders above what 2^17 additions
can lose.  Images and planes: the project's parity bar, relative L2 1e-4 against fp64; test_parity prints the achieved figures
(on an MI355X 3.2e-8 to 4.7e-8 for slc2 and 4.7e-8 to 9.4e-8 for the DPCA magnitude)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _balance_numpy as ref  # noqa: E402
import _gmti_numpy as gref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4             # end to end (test_gpu_parity.py)
SUM_TOL = 1e-12


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.complex128) - b) / max(np.linalg.norm(b), 1e-300))


def _pair(n_az, n_rg, seed, noise=0.1):
    """Two correlated channels with a smooth gain and phase mismatch, [n_az x n_rg] complex64."""
    r = np.random.default_rng(seed)

    def cn(p):
        return np.sqrt(p / 2) * (r.standard_normal((n_az, n_rg)) + 1j * r.standard_normal((n_az, n_rg)))
    c = cn(1.0)
    i, j = np.arange(n_az)[:, None] / n_az, np.arange(n_rg)[None, :] / n_rg
    m = (1 + 0.3 * np.sin(2 * np.pi * i) * np.cos(np.pi * j)) * np.exp(1j * (0.8 * np.cos(2 * np.pi * j) + 0.5 * i))
    return (c + cn(noise)).astype(np.complex64), ((c + cn(noise)) / m).astype(np.complex64)


def _run(s1, s2, params, clip_power=np.inf, dpca=True, in_place=False, with_slc1=True):
    """The two entry points on device buffers, with the clip level given as a power.  Returns (ChannelBalance, slc2_out, dpca_mag)."""
    import sarx
    from sarx import balance as B
    ctx = sarx.default_context()
    n_az, n_rg = s1.shape
    cp = params.c_params(n_az, n_rg, clip_power)
    d1, d2 = ctx.to_device(s1), ctx.to_device(s2)
    out = d2 if in_place else ctx.alloc(s2.nbytes)
    dm = ctx.alloc(n_az * n_rg * 4) if dpca else None
    table, ws = ctx.alloc(B.table_bytes(cp, n_az, n_rg)), ctx.alloc(B.workspace_bytes(cp, n_az, n_rg))
    try:
        B.enqueue_estimate(ctx, d1.ptr, d2.ptr, n_az, n_rg, cp, table.ptr, ws.ptr)
        B.enqueue_apply(ctx, d1.ptr if (dpca or with_slc1) else None, d2.ptr, n_az, n_rg, cp, table.ptr, out.ptr, dm.ptr if dpca else None)
        raw = table.download(np.uint8, (table.nbytes,)).copy()
        img = out.download(np.complex64, (n_az, n_rg)).copy()
        plane = dm.download(np.float32, (n_az, n_rg)).copy() if dpca else None
    finally:
        for b in {d1, d2, out, table, ws} | ({dm} if dm is not None else set()):
            b.release()
    return B.ChannelBalance(raw, (n_az, n_rg), params.block, params.interp, clip_power), img, plane


def _check_table(cb, t):
    scale = np.sqrt(t["s11"] * t["s22"])
    assert np.all(np.abs(cb.s12 - t["s12"]) <= SUM_TOL * np.maximum(scale, 1e-300)), np.max(np.abs(cb.s12 - t["s12"]) / np.maximum(scale, 1e-300))
    np.testing.assert_allclose(cb.s11, t["s11"], rtol=SUM_TOL)
    np.testing.assert_allclose(cb.s22, t["s22"], rtol=SUM_TOL)
    np.testing.assert_array_equal(cb.counts, t["n"])
    np.testing.assert_array_equal(cb.valid, t["valid"])
    assert cb.n_valid == t["n_valid"]
    np.testing.assert_allclose(cb.weights, t["w"], rtol=1e-11)
    np.testing.assert_allclose(cb.coherence, t["coherence"], rtol=1e-6, atol=1e-7)        # stored as fp32
    assert abs(cb.global_weight - t["global_weight"]) <= 1e-11 * abs(t["global_weight"])
    assert cb.global_coherence == pytest.approx(t["global_coherence"], rel=1e-11)


SHAPES = [((64, 64), (16, 16)), ((96, 80), (32, 16)), ((1000, 777), (256, 64)), ((64, 64), (4096, 4096))]
_cache = {}


def _case(shape, block):
    """The pair and its restatements, computed once per shape."""
    key = (shape, block)
    if key not in _cache:
        s1, s2 = _pair(*shape, seed=shape[0] + 3 * shape[1] + block[0])
        _cache[key] = (s1, s2, {})
    return _cache[key]


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
@pytest.mark.parametrize("mode", ["ls", "phase"])
@pytest.mark.parametrize("shape,block", SHAPES, ids=["%dx%d-b%dx%d" % (s + b) for s, b in SHAPES])
def test_parity(shape, block, mode, interp):
    import sarx
    s1, s2, memo = _case(shape, block)
    if (mode, interp) not in memo:
        memo[(mode, interp)] = ref.balance(s1, s2, block, mode, interp, min_count=1)
    t = memo[(mode, interp)]
    p = sarx.BalanceParams(block=block, mode=mode, interp=interp, min_count=1)
    res = sarx.channel_balance(s1.T, s2.T, p, dpca_mag=True)             # the public call, host images [N_rg x N_az]
    assert res.slc2.shape == s2.T.shape and res.dpca_mag.shape == s2.T.shape and res.slc2.dtype == np.complex64
    assert (res.nb_az, res.nb_rg) == t["w"].shape == (ref.n_blocks(shape[0], block[0]), ref.n_blocks(shape[1], block[1]))
    _check_table(res, t)
    e_img, e_dm = rel_l2(res.slc2.T, t["slc2"]), rel_l2(res.dpca_mag.T, t["dpca_mag"])
    print(f"{shape} {block} {mode} {interp}: slc2 rel-L2 {e_img:.2e}, dpca_mag rel-L2 {e_dm:.2e}")
    assert e_img < TOL and e_dm < TOL
    i, j = np.array([0, shape[0] // 2, shape[0] - 1]), np.array([shape[1] - 1, shape[1] // 3, 0])
    np.testing.assert_allclose(res.coherence_at(i, j), ref.interpolate(t["coherence"], shape, block, interp)[i, j], rtol=1e-6)


def test_device_images_in_and_out():
    """DeviceArray inputs give device results of the same kind; in_place overwrites slc2's buffer; clip_db takes its level from the
    image's mean power."""
    import sarx
    from sarx.engine import DeviceArray
    ctx = sarx.default_context()
    shape, block = (96, 80), (32, 16)
    s1, s2, _ = _case(shape, block)
    p = sarx.BalanceParams(block=block, clip_db=6.0, min_count=1)
    clip = 10 ** 0.6 * float(np.mean(np.abs(s1.astype(np.complex128)) ** 2))
    t = ref.balance(s1, s2, block, "ls", "bilinear", clip, min_count=1)
    assert t["n"].sum() < s1.size                                           # the clip bites
    d1, d2 = DeviceArray(ctx.to_device(s1), shape), DeviceArray(ctx.to_device(s2), shape)
    res = sarx.channel_balance(d1, d2, p, dpca_mag=True)
    assert isinstance(res.slc2, DeviceArray) and res.slc2.shape == shape and res.slc2.buf is not d2.buf
    assert res.clip_power == pytest.approx(clip, rel=1e-12)
    _check_table(res, t)
    out = res.slc2.numpy()
    assert rel_l2(out, t["slc2"]) < TOL
    assert rel_l2(res.dpca_mag.download(np.float32, shape), t["dpca_mag"]) < TOL
    np.testing.assert_array_equal(d2.numpy(), s2)                           # out of place: the input is untouched
    res2 = sarx.channel_balance(d1, d2, p, in_place=True)
    assert res2.slc2 is d2 and res2.dpca_mag is None
    np.testing.assert_array_equal(d2.numpy(), out)
    host = sarx.channel_balance(s1.T, s2.T, p)
    np.testing.assert_array_equal(host.slc2.T, out)
    with pytest.raises(sarx.SarxError, match="balance"):
        sarx.channel_balance(s1.T * 0, s2.T, p)
    for b in (res.slc2, res.dpca_mag, d1, d2):
        b.release()


def test_counts_and_validity():
    import sarx
    shape, block = (96, 80), (32, 16)
    s1, s2 = (x.copy() for x in _case(shape, block)[:2])
    s2[32:64, 16:32] = 0                                                    # an all-zero block (1, 1)
    s1[64:96, 48:64] *= 40.0                                                # block (2, 3): most of it over the clip level below
    s1[64:66, 48:64] /= 40.0                                                # ... except two rows: 32 pixels, below min_count
    pw = np.sort(np.concatenate([ref.power_f32(s1).ravel(), ref.power_f32(s2).ravel()]).astype(np.float64))
    k = int(np.searchsorted(pw, 6.0))
    gaps = pw[k + 1:k + 200] / pw[k:k + 199]
    g = k + int(np.argmax(gaps))
    clip = float(np.float32(np.sqrt(pw[g] * pw[g + 1])))
    assert not np.any(np.abs(pw - clip) <= 1e-5 * clip), "a pixel's power lies within 1e-5 of the clip level"
    for clip_power, min_count in ((np.inf, 1), (clip, 64), (clip, 1)):
        p = sarx.BalanceParams(block=block, mode="ls", interp="bilinear", min_count=min_count)
        cb, img, dm = _run(s1, s2, p, clip_power)
        t = ref.balance(s1, s2, block, "ls", "bilinear", clip_power, min_count)
        np.testing.assert_array_equal(cb.counts, t["n"])
        np.testing.assert_array_equal(cb.valid, t["valid"])
        _check_table(cb, t)
        assert not cb.valid[1, 1] and cb.s22[1, 1] == 0.0 and cb.coherence[1, 1] == 0.0
        assert cb.weights[1, 1] == cb.global_weight                         # bit for bit the header's weight
        if clip_power != np.inf:
            assert cb.counts.sum() < s1.size and cb.counts[2, 3] == t["n"][2, 3] < 64
            assert cb.valid[2, 3] == (min_count == 1)
            if min_count == 64:
                assert cb.weights[2, 3] == cb.global_weight
        assert rel_l2(img, t["slc2"]) < TOL and rel_l2(dm, t["dpca_mag"]) < TOL
        assert np.isfinite(cb.raw.view(np.uint8)[64:].view(sarx.balance.RECORD_DTYPE)["w_re"]).all()
    none, img, _ = _run(s1 * 0, s2, sarx.BalanceParams(block=block), dpca=False)       # no valid block: weight 1, n_valid 0
    assert none.n_valid == 0 and none.global_weight == 1.0 and (none.weights == 1.0).all()
    np.testing.assert_array_equal(img, s2)


@pytest.mark.parametrize("shape,block", [((96, 80), (32, 16)), ((1000, 777), (256, 64))], ids=["96x80", "1000x777"])
def test_determinism_and_aliasing(shape, block):
    import sarx
    s1, s2, _ = _case(shape, block)
    p = sarx.BalanceParams(block=block, min_count=1)
    a, img_a, dm_a = _run(s1, s2, p)
    b, img_b, dm_b = _run(s1, s2, p)
    assert a.raw.tobytes() == b.raw.tobytes() and img_a.tobytes() == img_b.tobytes() and dm_a.tobytes() == dm_b.tobytes()
    c, img_c, dm_c = _run(s1, s2, p, in_place=True)
    assert c.raw.tobytes() == a.raw.tobytes() and img_c.tobytes() == img_a.tobytes() and dm_c.tobytes() == dm_a.tobytes()
    d, img_d, _ = _run(s1, s2, p, dpca=False, with_slc1=False)               # slc1 = NULL without dpca_mag
    assert d.raw.tobytes() == a.raw.tobytes() and img_d.tobytes() == img_a.tobytes()
    e, img_e, _ = _run(s1, s2, p, dpca=False, in_place=True)
    assert img_e.tobytes() == img_a.tobytes()


LAM, V, LAG = 0.031, 7500.0, 1.0 / 6000.0


def test_mismatch_fixture():
    """256 x 192, default_rng(7): unit clutter common to both channels, noise at -30 dB, slc2 = (c + n2) / (g e^{j phi}) with a gain
    and phase no scalar follows, three 25 dB movers.  Block (32, 32), LS, bilinear, clip 10^1.2.  Restatement (CPU prototype of the
    semantics): residue -22.1 dB against -7.2 dB under one least-squares weight (14.9 dB), movers within 0.6 dB of |A - A e^{-jp}|^2,
    first mover 1.8 dB down without the clip."""
    import sarx
    s1, s2 = ref.mismatch_fixture()
    n_az, n_rg = s1.shape
    glob = ref.balance(s1, s2, (4096, 4096), "ls", "nearest", ref.FIXTURE_CLIP)
    blk = ref.balance(s1, s2, ref.FIXTURE_BLOCK, "ls", "bilinear", ref.FIXTURE_CLIP, min_count=256)
    noclip = ref.balance(s1, s2, ref.FIXTURE_BLOCK, "ls", "bilinear", np.inf, min_count=256)
    r_glob, r_blk = ref.residue_db(s1, glob["slc2"]), ref.residue_db(s1, blk["slc2"])
    want = np.array([ref.mover_expected_db(p) for _, p in ref.FIXTURE_MOVERS])
    m_blk = np.array(ref.mover_db(s1, blk["slc2"]))
    print(f"restatement: residue global LS {r_glob:.2f} dB, block {r_blk:.2f} dB; movers {m_blk.round(2)} for {want.round(2)}; "
          f"first mover without clip {ref.mover_db(s1, noclip['slc2'])[0]:.2f}")
    assert r_glob - r_blk >= 12.0
    assert np.all(np.abs(m_blk - want) <= 1.0)
    assert want[0] - ref.mover_db(s1, noclip["slc2"])[0] > 1.0

    p = sarx.BalanceParams(block=ref.FIXTURE_BLOCK, mode="ls", interp="bilinear", min_count=256)
    cb, img, dm = _run(s1, s2, p, ref.FIXTURE_CLIP)
    _check_table(cb, blk)
    r_gpu, m_gpu = ref.residue_db(s1, img), np.array(ref.mover_db(s1, img))
    print(f"gpu: residue {r_gpu:.3f} dB ({r_gpu - r_blk:+.1e}), movers {m_gpu.round(3)}")
    assert abs(r_gpu - r_blk) <= 0.1 and np.all(np.abs(m_gpu - m_blk) <= 0.1)
    ra, ca = 5e5 + 0.25 * np.arange(n_rg), 1.2 * (np.arange(n_az) - n_az / 2)
    rep = sarx.gmti_detect(s1.T, img.T, ra, ca, wavelength_m=LAM, platform_speed_mps=V, lag_s=LAG, cal_phase=0.0)
    cells = list(zip(rep.detections["i"].tolist(), rep.detections["j"].tolist()))
    o = gref.cfar(blk["dpca_mag"].astype(np.float32))
    missing, extra = gref.compare(cells, o)
    assert not missing and not extra, (missing, extra, cells, o["cells"])
    for (mi, mj), _ in ref.FIXTURE_MOVERS:
        assert (mi, mj) in cells, ((mi, mj), cells)


def test_focus_ati_dpca_with_balance():
    """256 x 256 noise echoes, channel 2 scaled by a smooth mismatch before focusing: the call with balance= equals
    channel_balance + ati_dpca on its own images bit for bit, and the call without it is what it was (the fused product stage)."""
    import sarx
    from oracle import csa_oracle as orc
    n = 256
    args = orc.focus_args(orc.scaled_radar(n, n))
    r = np.random.default_rng(11)
    r1 = (r.standard_normal((n, n)) + 1j * r.standard_normal((n, n))).astype(np.complex64)
    i, j = np.arange(n)[:, None] / n, np.arange(n)[None, :] / n
    r2 = (r1 * (1 + 0.2 * np.sin(2 * np.pi * i)) * np.exp(1j * (0.5 * np.cos(2 * np.pi * j) + 0.3 * i)) +
          0.05 * (r.standard_normal((n, n)) + 1j * r.standard_normal((n, n)))).astype(np.complex64)
    p = sarx.BalanceParams(block=(64, 32), clip_db=12.0)
    base = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False)
    assert base["fused_products"] and "balance" not in base
    np.testing.assert_array_equal(base["slc1"], sarx.sar_focus_csa(r1, *args)[0])
    np.testing.assert_array_equal(base["slc2"], sarx.sar_focus_csa(r2, *args)[0])
    two = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, unmasked_phase=True)
    for key in ("slc1_mag", "dpca_mag", "ati_phase_masked"):
        np.testing.assert_array_equal(base[key], two[key])

    bal = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, balance=p)
    assert not bal["fused_products"]
    cb = sarx.channel_balance(base["slc1"], base["slc2"], p)
    assert bal["balance"].raw.tobytes() == cb.raw.tobytes()
    assert bal["balance"].clip_power == cb.clip_power and bal["balance"].n_valid == 32
    np.testing.assert_array_equal(bal["slc1"], base["slc1"])
    np.testing.assert_array_equal(bal["slc2"], cb.slc2)
    prod = sarx.ati_dpca(base["slc1"], cb.slc2, mask_frac=0.05, cal_phase=0.0)
    for key in ("slc1_mag", "dpca_mag", "ati_phase_masked"):
        np.testing.assert_array_equal(bal[key], prod[key], err_msg=key)
    assert abs(bal["sum_interf"] - prod["sum_interf"]) <= 1e-9 * abs(prod["sum_interf"])
    assert np.mean(bal["dpca_mag"] ** 2) < np.mean(base["dpca_mag"] ** 2)       # a least-squares fit per block: never worse
    t = ref.balance(base["slc1"].T, base["slc2"].T, p.block, "ls", "bilinear", cb.clip_power, min_count=64 * 32 // 4)
    _check_table(cb, t)
    assert rel_l2(cb.slc2.T, t["slc2"]) < TOL

    det = sarx.GmtiParams(pfa=1e-3, max_detections=8192)
    full = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, balance=p, detect=det)
    alone = sarx.gmti_detect(base["slc1"], cb.slc2, base["range_axis"], base["cross_range"], wavelength_m=args[0],
                             platform_speed_mps=args[5], lag_s=1.0 / args[4], pfa=1e-3, cal_phase=0.0, max_detections=8192)
    assert full["detections"].detections.tobytes() == alone.detections.tobytes()
