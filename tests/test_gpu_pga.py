"""The phase-gradient autofocus on the device (include/sarx_pga.h, csrc/pga.hip, sarx/pga.py) against the NumPy fp64 restatement
(tests/_pga_numpy.py): the apply launch, the whole estimate-and-apply chain, a padded stack against its frames one by one, and the
Python routes.  The inputs are the guarded cases of tests/test_pga.py, each computed once per process.

Bounds of the chain (measured on the MI355X over every case below, the largest deviation from the restatement; asserted at four times
that, which covers box-to-box code-generation differences of the fp32 transform; the caps of 1e-3 rad and 1e-4 relative are where
something other than rounding is wrong):
    phi_tot, all bins      measured 2.99e-7 rad   bound 1.2e-6 rad
    rms_phase              measured 1.94e-7 rad   bound 7.8e-7 rad
    s2 (relative)          measured 3.22e-7       bound 1.3e-6
    s4 (relative)          measured 9.13e-7       bound 3.7e-6
    d_out (relative L2)    measured 2.46e-7       bound 1e-4 (the project's parity bar, as the issue sets it)
    apply (relative L2)    measured 2.32e-7       bound 1e-4 (the project's parity bar, as the issue sets it)"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pga_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu

PARITY = 1e-4
PHI_BOUND = min(4 * 2.99e-7, 1e-3)
RMS_BOUND = min(4 * 1.94e-7, 1e-3)
S2_BOUND = min(4 * 3.22e-7, 1e-4)
S4_BOUND = min(4 * 9.13e-7, 1e-4)
CHAIN_CASES = [(s, k, c, False) for s, k, c in ref.FULL_CASES + ref.EXTRA_CASES] + [(s, k, 0.0, True) for s, k in ref.BAND_CASES]
APPLY_SHAPES = [(s[0], s[1]) for s in ref.MAIN_SHAPES + ref.EXTRA_SHAPES]


def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.complex128) - b) / np.linalg.norm(b))


def _params(c):
    import sarx
    return sarx.PgaParams(n_iter=ref.N_ITER, half_widths=c["half_widths"], min_contrast=c["min_contrast"], power_floor=c["power_floor"])


@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("n_az,n_rg", APPLY_SHAPES, ids=[f"{a}x{b}" for a, b in APPLY_SHAPES])
def test_apply_against_the_fp64_transform(n_az, n_rg, sign):
    import sarx
    img = ref.scene(n_az, n_rg, min(3, n_rg), 11)
    phi = ref.error("cubic_sine", n_az) + 40.0 * np.linspace(-1, 1, n_az) ** 2          # many revolutions: the reduction is exercised
    got = sarx.apply_azimuth_phase(img, phi, sign=sign)
    e = _rel_l2(got, ref.apply(img, phi, sign))
    print(f"apply {n_az} x {n_rg}, sign {sign:+d}: relative L2 {e:.3e}")
    assert got.dtype == np.complex64 and got.shape == img.shape
    assert e <= PARITY


@pytest.mark.parametrize("shape,kind,min_contrast,band", CHAIN_CASES,
                         ids=[ref.case_id(s, k, c) + ("-band" if b else "") for s, k, c, b in CHAIN_CASES])
def test_chain_against_the_restatement(shape, kind, min_contrast, band):
    import sarx
    c = ref.case(shape, kind, min_contrast, band)
    assert ref.guards_hold(c["guards"])
    res = sarx.pga(c["blur"], _params(c))
    want = c["records"]
    d_phi = float(np.abs(res.phase - c["phi"]).max())
    d_rms = float(np.abs(res.records["rms_phase"] - want["rms_phase"]).max())
    d_s2 = float(np.abs(res.records["s2"] / want["s2"] - 1.0).max())
    d_s4 = float(np.abs(res.records["s4"] / want["s4"] - 1.0).max())
    d_out = _rel_l2(res.image, c["out"])
    print(f"chain: phi_tot {d_phi:.3e} rad, rms_phase {d_rms:.3e} rad, s2 {d_s2:.3e}, s4 {d_s4:.3e}, d_out {d_out:.3e}")
    assert res.records.shape == (ref.N_ITER + 1,) and res.phase.shape == (shape[0],) and res.image.shape == c["blur"].shape
    np.testing.assert_array_equal(res.records["n_cols_used"], want["n_cols_used"])
    np.testing.assert_array_equal(res.records["n_bins_supported"], want["n_bins_supported"])
    assert d_phi <= PHI_BOUND and d_rms <= RMS_BOUND
    assert d_s2 <= S2_BOUND and d_s4 <= S4_BOUND
    assert d_out <= PARITY
    np.testing.assert_allclose(res.sharpness, want["s4"] / want["s2"] ** 2, rtol=S4_BOUND + 2 * S2_BOUND)


def _stack():
    """Three frames of 128 x 17 in one buffer with ld = n_rg + 5 and a padded frame stride; (host buffer, frames, ld, stride)."""
    n_az, n_rg = 128, 17
    ld, stride = n_rg + 5, 128 * (n_rg + 5) + 37
    frames = [ref.case((n_az, n_rg, 6), k, 0.0)["blur"] for k in ("cubic_sine", "quadratic")]
    frames.append(ref.apply(ref.scene(n_az, n_rg, 6, 1), 0.5 * ref.error("quadratic", n_az), +1).astype(np.complex64))
    host = np.full(2 * stride + n_az * ld, np.nan + 1j * np.nan, np.complex64)
    for f, img in enumerate(frames):
        host[f * stride:f * stride + n_az * ld].reshape(n_az, ld)[:, :n_rg] = img
    return host, frames, ld, stride


def test_stack_equals_its_frames_and_runs_repeat():
    import sarx
    K = importlib.import_module("sarx.pga")
    ctx = sarx.default_context()
    host, frames, ld, stride = _stack()
    n_az, n_rg, nf = 128, 17, 3
    prm = sarx.PgaParams(n_iter=ref.N_ITER, half_widths=ref.default_half_widths(n_az, ref.N_ITER))
    cp = prm.c_params(n_az)
    n_rec = ref.N_ITER + 1
    d_in = ctx.to_device(host)
    bufs = [d_in]
    try:
        runs = []
        for _ in range(2):
            d_out, d_ph, d_rec = ctx.alloc(host.nbytes), ctx.alloc(nf * n_az * 8), ctx.alloc(nf * n_rec * 32)
            d_ws = ctx.alloc(K.workspace_bytes(cp, n_az, n_rg, ld, nf, stride))
            bufs += [d_out, d_ph, d_rec, d_ws]
            check = ctx.lib.sarx_memset(ctx.h, d_out.ptr, 0, host.nbytes)
            assert check == 0
            K.enqueue(ctx, d_in.ptr, d_out.ptr, n_az, n_rg, ld, nf, stride, cp, d_ph.ptr, d_rec.ptr, d_ws.ptr)
            runs.append((np.array(d_out.download(np.complex64, host.shape)), np.array(d_ph.download(np.float64, (nf, n_az))),
                         np.array(d_rec.download(np.uint8, (nf * n_rec * 32,)))))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))                    # two runs: the same bits
        out, ph, rec = runs[0]
        rec = rec.view(K.RECORD_DTYPE).reshape(nf, n_rec)
        for f, img in enumerate(frames):
            single = sarx.pga(img, prm)
            got = out[f * stride:f * stride + n_az * ld].reshape(n_az, ld)[:, :n_rg]
            assert got.tobytes() == single.image.tobytes(), f                           # frame f of the stack = that frame alone
            assert ph[f].tobytes() == single.phase.tobytes() and rec[f].tobytes() == single.records.tobytes(), f
        want = ref.case((n_az, n_rg, 6), "cubic_sine", 0.0)
        np.testing.assert_array_equal(rec[0]["n_cols_used"], want["records"]["n_cols_used"])
        assert np.abs(ph[0] - want["phi"]).max() <= PHI_BOUND
        # as a stack through the Python route
        res = sarx.pga(np.stack(frames), prm)
        assert res.image.shape == (nf, n_az, n_rg) and res.phase.tobytes() == ph.tobytes() and res.records.tobytes() == rec.tobytes()
    finally:
        for b in bufs:
            b.release()


def test_axis_1_equals_axis_0_of_the_transposed_image():
    import sarx
    n_az, n_rg = 64, 96
    img = ref.apply(ref.scene(n_az, n_rg, 9, 4), ref.error("quadratic", n_az), +1).astype(np.complex64)
    prm = sarx.PgaParams(n_iter=3)
    a = sarx.pga(img, prm, axis=0)
    b = sarx.pga(np.ascontiguousarray(img.T), prm, axis=1)
    assert b.image.shape == (n_rg, n_az)
    assert np.ascontiguousarray(b.image.T).tobytes() == a.image.tobytes()
    assert a.phase.tobytes() == b.phase.tobytes() and a.records.tobytes() == b.records.tobytes()
    phi = ref.error("cubic_sine", n_az)
    x = sarx.apply_azimuth_phase(img, phi, sign=1)
    y = sarx.apply_azimuth_phase(np.ascontiguousarray(img.T), phi, sign=1, axis=1)
    assert np.ascontiguousarray(y.T).tobytes() == x.tobytes()
    with pytest.raises(ValueError, match="32"):
        sarx.pga(np.zeros((17, 64), np.complex64), prm, axis=1)


def test_device_input_and_estimated_phase_applied_to_another_frame():
    import sarx
    ctx = sarx.default_context()
    c = ref.case((256, 33, 10), "quadratic", 0.0)
    prm = _params(c)
    host = sarx.pga(c["blur"], prm)
    d = ctx.to_device(c["blur"])
    try:
        dev = sarx.pga(sarx.DeviceArray(d, c["blur"].shape, owner=False), prm)
        try:
            assert np.array(dev.image.download(np.complex64, c["blur"].shape)).tobytes() == host.image.tobytes()
            assert dev.phase.tobytes() == host.phase.tobytes()
        finally:
            dev.release()
    finally:
        d.release()
    # the phase estimated here, applied by the apply step alone: the output of the call (it always transforms the input)
    again = sarx.apply_azimuth_phase(c["blur"], host.phase, sign=-1)
    assert again.tobytes() == host.image.tobytes()
    # one phase for every frame of a stack, and one per frame
    two = np.stack([c["blur"], c["clean"].astype(np.complex64)])
    both = sarx.apply_azimuth_phase(two, host.phase, sign=-1)
    assert both[0].tobytes() == host.image.tobytes()
    each = sarx.apply_azimuth_phase(two, np.stack([host.phase, np.zeros(256)]), sign=-1)
    assert each[0].tobytes() == host.image.tobytes() and _rel_l2(each[1], two[1]) <= PARITY


def test_refusals_on_the_device():
    import sarx
    from sarx import _ffi
    K = importlib.import_module("sarx.pga")
    ctx = sarx.default_context()
    cp = sarx.PgaParams(n_iter=2).c_params(64)
    buf = ctx.alloc(1 << 16)
    try:
        p = buf.ptr
        img = 64 * 4 * 8
        ok = (p, p + 4096, 64, 4, 4, 1, 0, cp, p + 8192, p + 12288, p + 16384)
        K.enqueue(ctx, *ok)
        for bad in ((p, p + img - 8) + ok[2:],                           # d_out overlaps d_in
                    (p, p) + ok[2:],
                    ok[:8] + (p + 4096 + 8, p + 12288, p + 16384),       # phase inside d_out
                    ok[:10] + (p + 12288,),                              # workspace on the records
                    (p + 4,) + ok[1:],                                   # misaligned
                    ok[:10] + (None,)):
            with pytest.raises(_ffi.SarxError):
                K.enqueue(ctx, *bad)
        with pytest.raises(_ffi.SarxError):
            K.enqueue_apply(ctx, p, p + 8, 64, 4, 4, 1, 0, p + 8192, 0, -1)
        with pytest.raises(_ffi.SarxError):
            K.enqueue_apply(ctx, p, p + 4096, 64, 4, 4, 1, 0, p + 8192, 0, 2)
        with pytest.raises(_ffi.SarxError):
            K.enqueue_apply(ctx, p, p + 4096, 64, 4, 4, 2, 64 * 4, p + 8192, 63, 1)
        ctx.sync()
    finally:
        buf.release()


def test_tdbp_autofocus_passes_its_frame_through_pga():
    """pga=None returns today's bytes (the existing tests hold that); with parameters the returned frame is sarx.pga of it."""
    import sarx
    import _tdbp_search_numpy as ts
    sc = ts.recovery_scene()
    k = sc["k"]
    nx, ny = 64, 128
    d_raw, t0, n, v_tgt = sarx.run_physics_spotlight(sc["targets"], sc["t_vec"], sc["pos"], sc["vel"], sc["heading_deg"], sc["speed"],
                                                     sc["l_ant"], consts=k, device=True)
    try:
        common = dict(v0=v_tgt, half_span=6.0, n=3, consts=k)
        prm = sarx.PgaParams(n_iter=2)
        _, plain, _ = sarx.tdbp_autofocus(d_raw, sc["pos"], sc["vel"], t0, n, sc["t_vec"], sc["swath"], nx, ny, **common)
        _, both, _ = sarx.tdbp_autofocus(d_raw, sc["pos"], sc["vel"], t0, n, sc["t_vec"], sc["swath"], nx, ny, pga=prm, **common)
        _, turned, _ = sarx.tdbp_autofocus(d_raw, sc["pos"], sc["vel"], t0, n, sc["t_vec"], sc["swath"], nx, ny, pga=prm, pga_axis=1, **common)
        with pytest.raises(ValueError):
            sarx.tdbp_autofocus(d_raw, sc["pos"], sc["vel"], t0, n, sc["t_vec"], sc["swath"], nx, ny, pga=prm, d_image=d_raw, **common)
    finally:
        d_raw.release()
    assert plain.shape == both.shape == (ny, nx) and both.dtype == np.complex128
    assert np.array_equal(both, sarx.pga(plain.astype(np.complex64), prm).image.astype(np.complex128))
    assert np.array_equal(turned, sarx.pga(plain.astype(np.complex64), prm, axis=1).image.astype(np.complex128))
