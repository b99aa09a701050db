"""Guard bands and poison around every device entry point (tests/_guard.py): what a kernel does OUTSIDE its output and which
promised bytes it never writes.  One table (CASES), one test.  For every case all device arguments are GuardedBuffers; the call
runs once with every output poisoned (0xFF) and once zeroed; the promised bytes of the two results must be bit-identical and
finite, bytes the header leaves alone must still be 0xFF, every zone must be clean and every const input unchanged.  Shapes that
no parity test covers are also compared with their oracle at the neighbouring test's tolerance (PASS_TOL per pass, TOL end to
end; no new tolerance).  Teeth are shown in tests/test_guard_helper.py on fake kernels; no real kernel is broken here.

Determinism: every entry point below turned out bit-reproducible between the two runs, so none falls back to a tolerance."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmti_numpy as gref  # noqa: E402
import _refocus_numpy as rref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402
from sarx import _ffi  # noqa: E402  (ctypes tables only: nothing is loaded at import)

pytestmark = pytest.mark.gpu

TOL = 1e-4            # end to end (test_gpu_parity.py)
PASS_TOL = 5e-6       # per pass (test_each_pass)

# entry points that no one-GPU case can reach, each with its reason
EXCLUDED = {}


def _rand(shape, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(np.complex64)


def _randf(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _clean(ctx, call, inputs, outputs, promised=None, dtypes=None):
    findings, res = guarded_run(call, inputs, outputs, promised, dtypes, sync=ctx.sync)
    assert not findings, findings
    return res["poisoned"]


def _zones_clean(*bufs):
    for b in bufs:
        assert b.check_zones() == [], b.check_zones()


def _release(*bufs):
    for b in bufs:
        if b is not None:
            b.release()


F32, F64 = np.float32, np.float64
RANGE_IDS = (2, 3, 23, 100, 101, 12, 13)


# ---- sarx_csa_pass -----------------------------------------------------------------------------------------------------
def csa_pass(sx, ctx, orc, n_az, n_rg, ids, parity=False, range_cus=0, flags=0, az_waves=None, mp=None):
    """az_waves: the case is about the wave-private 128-point azimuth tiles of n_az = 16384 (az_wave.hip): 1 or 4 waves per
    workgroup (SARX_AZ_WAVES, read at plan creation; n_rg must be a multiple of 32 x that).  That they ran is shown against a
    plan with SARX_AZ_IMPL=0 (az_tile_kernel): other order of additions, so equal to rounding (test_gpu_az_wave.py's 1e-6), not bit for bit."""
    z = zone_bytes(n_rg * 8)
    if parity:
        raw, k = orc.point_scene(n_az, n_rg, seed=n_az + n_rg, clutter_db=-15.0)
        args = orc.focus_args(k)
        _, _, _, (s1, s2, s3, s4) = orc.sar_focus_csa(raw, *args, return_stages=True)
        src = {1: (raw, s1), 2: (s1, s2), 3: (s2, s3), 4: (s3, s4), 23: (s1, s3)}
    else:
        args = orc.focus_args(orc.scaled_radar(n_az, n_rg))
        x = _rand((n_az, n_rg), 7 * n_az + n_rg)
    tile_plan = None
    if az_waves:
        assert n_az == 16384 and n_rg % (32 * az_waves) == 0
        mp.setenv("SARX_AZ_IMPL", "0")
        tile_plan = sx.CsaPlan(ctx, n_az, n_rg, *args, flags=flags)
        mp.setenv("SARX_AZ_IMPL", "1")
        mp.setenv("SARX_AZ_WAVES", str(az_waves))
    plan = sx.CsaPlan(ctx, n_az, n_rg, *args, flags=flags)
    if az_waves:
        mp.delenv("SARX_AZ_IMPL")
        mp.delenv("SARX_AZ_WAVES")
    d_in, d_out = GuardedBuffer(ctx, n_az * n_rg * 8, z), GuardedBuffer(ctx, n_az * n_rg * 8, z)
    if range_cus:
        ctx.set_range_cus(range_cus)
    try:
        for pid in ids:
            host = np.ascontiguousarray(src[pid][0].astype(np.complex64)) if parity and pid in src else \
                (x if not parity else _rand((n_az, n_rg), pid))
            got = _clean(ctx, lambda: plan.run_pass(pid, d_in, d_out), {"in": (d_in, host)}, {"out": d_out}, dtypes={"out": F32})
            if parity and pid in src:
                err = orc.rel_l2(got["out"].view(np.complex64).reshape(n_az, n_rg), src[pid][1])
                print(f"pass {pid} {n_az}x{n_rg}: rel-L2 {err:.2e}")
                assert err < PASS_TOL, (pid, err)
            if tile_plan is not None:
                tile_plan.run_pass(pid, d_in, d_out)
                ctx.sync()
                old = d_out.download(np.complex64)
                new = got["out"].view(np.complex64)
                assert not np.array_equal(new, old), f"pass {pid}: the wave-private kernel did not run"
                assert orc.rel_l2(new, old) < 1e-6, pid
            if pid in RANGE_IDS:                                 # documented in-place form: equal to out-of-place bit for bit
                d_in.upload(host)
                plan.run_pass(pid, d_in, d_in)
                ctx.sync()
                _zones_clean(d_in)
                assert np.array_equal(d_in.download(), got["out"]), f"pass {pid} in place differs"
    finally:
        ctx.set_range_cus(0)
        plan.close()
        if tile_plan is not None:
            tile_plan.close()
        _release(d_in, d_out)


# ---- sarx_csa_focus_dev --------------------------------------------------------------------------------------------------
def focus(sx, ctx, orc, n_az, n_rg, flags=0, slab=None, parity=False, mp=None):
    z = zone_bytes(max(n_az, n_rg) * 8)
    x = _rand((n_az, n_rg), n_az * 131 + n_rg)
    args = orc.focus_args(orc.scaled_radar(max(n_az, 16), max(n_rg, 16)))
    if slab is not None:
        mp.setenv("SARX_SLAB_MIB", str(slab))
    plan = sx.CsaPlan(ctx, n_az, n_rg, *args, flags=flags)
    if slab is not None:
        mp.delenv("SARX_SLAB_MIB")
    d_in, d_out = GuardedBuffer(ctx, x.nbytes, z), GuardedBuffer(ctx, x.nbytes, z)
    try:
        got = _clean(ctx, lambda: plan.focus_dev(d_in, d_out), {"phist": (d_in, x)}, {"image": d_out}, dtypes={"image": F32})
        if parity:
            img = got["image"].view(np.complex64).reshape((n_rg, n_az) if flags & _ffi.OUT_RG_MAJOR else (n_az, n_rg))
            ref = orc.sar_focus_csa(x, *args)[0]
            err = orc.rel_l2(img if flags & _ffi.OUT_RG_MAJOR else img.T, ref)
            print(f"focus {n_az}x{n_rg}: rel-L2 {err:.2e}")
            assert err < TOL, err
    finally:
        plan.close()
        _release(d_in, d_out)


# ---- fused epilogues: look slot, max slot, ATI planes ------------------------------------------------------------------------
def epilogues(sx, ctx, orc, n_az, n_rg, looks=(), keep=True):
    z = zone_bytes(n_rg * 8)
    px = n_az * n_rg
    r = np.random.default_rng(px)
    x1 = (r.standard_normal((n_az, n_rg), dtype=F32) + 1j * r.standard_normal((n_az, n_rg), dtype=F32)).astype(np.complex64)
    x2 = (x1 * np.complex64(0.9 + 0.1j)).astype(np.complex64)
    x2[1:] += np.complex64(0.05) * x1[:-1]
    args = orc.focus_args(orc.scaled_radar(n_az, n_rg))
    plan = sx.CsaPlan(ctx, n_az, n_rg, *args, flags=_ffi.FUSE_RANGE)
    d1, d2 = GuardedBuffer(ctx, px * 8, z), GuardedBuffer(ctx, px * 8, z)
    s1, s2 = GuardedBuffer(ctx, px * 8, z), GuardedBuffer(ctx, px * 8, z)
    d_max = GuardedBuffer(ctx, _ffi.MAX_SLOT_BYTES)
    planes = {k: GuardedBuffer(ctx, px * 4, z) for k in ("ati_phase_masked", "slc1_mag", "dpca_mag")}
    slot = None
    try:
        plan.set_max_slot(d_max)
        got = _clean(ctx, lambda: plan.focus_dev(d1, s1), {"phist": (d1, x1)}, {"slc1": s1, "max": d_max},
                     dtypes={"slc1": F32, "max": F32})
        plan.set_max_slot(None)
        shards = got["max"].view(F32).reshape(256, 32)
        assert not shards[:, 1:].any()
        mx = np.abs(got["slc1"].view(np.complex64)).max()
        assert abs(float(shards[:, 0].max()) - mx) <= 2e-7 * mx          # test_fused_max_and_masked_ati's statement
        for L in looks:
            nslot = (n_az // L) * (n_rg // L)
            slot = GuardedBuffer(ctx, nslot * 4, z)
            plan.set_look_slot(L, slot.ptr)
            g2 = _clean(ctx, lambda: plan.focus_dev(d1, s2), {"phist": (d1, x1)}, {"image": s2, "look": slot},
                        dtypes={"image": F32, "look": F32})
            plan.set_look_slot(L, None)
            assert np.array_equal(g2["image"], got["slc1"])
            img = g2["image"].view(np.complex64).reshape(n_az, n_rg).astype(np.complex128)
            ref = (np.abs(img) ** 2).reshape(n_az // L, L, n_rg // L, L).mean(axis=(1, 3))
            assert orc.rel_l2(g2["look"].view(F32).reshape(ref.shape), ref) < 1e-6      # test_fused_look_slot's bar
            slot.release()
            slot = None
        h_s1, h_max = got["slc1"].copy(), got["max"].copy()
        plan.set_ati(s1, d_max, 0.05, 0.3, planes["ati_phase_masked"], planes["slc1_mag"], planes["dpca_mag"], keep_image=keep)
        outs = dict(planes, slc2=s2)
        g3 = _clean(ctx, lambda: plan.focus_dev(d2, s2), {"phist": (d2, x2), "slc1": (s1, h_s1), "max": (d_max, h_max)}, outs,
                    promised={"slc2": px * 8 if keep else None}, dtypes={k: F32 for k in outs})
        plan.set_ati(None)
        assert 0 < np.count_nonzero(g3["ati_phase_masked"].view(F32)) < px
        # against the separate launch on the two finished images (bit for bit, test_ati_products_fused_into_second_focus)
        plan.focus_dev(d2, s2)
        ref = {k: GuardedBuffer(ctx, px * 4, z) for k in ("ati_phase", "slc1_mag", "dpca_mag")}
        ctx.ati_dpca_masked(s1, s2, px, 0.3, d_max, 0.05, ref)
        ctx.sync()
        for a, b in (("ati_phase_masked", "ati_phase"), ("slc1_mag", "slc1_mag"), ("dpca_mag", "dpca_mag")):
            assert np.array_equal(g3[a], ref[b].download()), a
        _zones_clean(*ref.values(), s1, s2, d_max)
        _release(*ref.values())
    finally:
        plan.close()
        _release(d1, d2, s1, s2, d_max, slot, *planes.values())


# ---- element-wise products ---------------------------------------------------------------------------------------------------
ATI_REQ = ("ati_phase", "slc1_mag", "dpca_mag")
ATI_OPT = {"ati_interf": 8, "dpca_diff": 8, "slc2_mag": 4, "slc1_phase": 4, "slc2_phase": 4, "dpca_phase": 4}


def products(sx, ctx, orc, n, alone=True):
    from sarx import noise
    a, b = _rand((n,), n), _rand((n,), n + 1)
    s1, s2 = guarded(ctx, a), guarded(ctx, b)
    bufs = {k: GuardedBuffer(ctx, n * 4) for k in ATI_REQ}
    bufs.update({k: GuardedBuffer(ctx, n * w) for k, w in ATI_OPT.items()})
    slot = np.zeros(_ffi.MAX_SLOT_BYTES // 4, F32)
    slot[::32] = np.abs(a).max() * np.linspace(0.2, 1.0, 256, dtype=F32)
    d_slot = guarded(ctx, slot)
    ins = {"slc1": (s1, a), "slc2": (s2, b)}
    try:
        sets = [tuple(ATI_OPT)] + ([(k,) for k in ATI_OPT] + [()] if alone else [])
        for opt in sets:                                             # each optional plane alone, none, and all together
            outs = {k: bufs[k] for k in ATI_REQ + opt}
            for k in ATI_OPT:
                bufs[k].poison()
            g = _clean(ctx, lambda: ctx.ati_dpca(s1, s2, n, 0.3, outs), ins, outs, dtypes={k: F32 for k in outs})
            for k in ATI_OPT:                                        # planes not requested are not touched
                if k not in opt:
                    assert (bufs[k].download() == 0xFF).all()
            mx, sm = g["return"]
            assert mx == np.float64(np.abs(g["slc1_mag"].view(F32)).max()) and np.isfinite([sm.real, sm.imag]).all()
        ref = orc.ati_dpca(a.reshape(1, n), b.reshape(1, n), cal_phase=0.3)
        assert orc.rel_l2(g["slc1_mag"].view(F32), ref["slc1_mag"].reshape(-1)) < 1e-6          # test_ati_dpca_fixture's bars
        assert orc.rel_l2(g["dpca_mag"].view(F32), ref["dpca_mag"].reshape(-1)) < 1e-5
        outs = {k: bufs[k] for k in ATI_REQ}
        gm = _clean(ctx, lambda: ctx.ati_dpca_masked(s1, s2, n, 0.3, d_slot, 0.05, outs), dict(ins, max=(d_slot, slot)), outs,
                    dtypes={k: F32 for k in outs})
        mag1, thr = g["slc1_mag"].view(F32).astype(F64), 0.05 * float(slot.max())
        keepm, drop = mag1 > thr * (1 + 1e-6), mag1 < thr * (1 - 1e-6)       # a pixel within fp32 rounding of the threshold may go either way
        assert not gm["ati_phase"].view(F32)[drop].any()
        assert np.array_equal(gm["ati_phase"].view(F32)[keepm], g["ati_phase"].view(F32)[keepm])
        for k in ("slc1_mag", "dpca_mag"):
            assert np.array_equal(gm[k], g[k])
        # magnitude, mask_phase (and its aliased form), mask_phase_frac
        d_mag = bufs["slc2_mag"]
        gg = _clean(ctx, lambda: ctx.magnitude(s1, d_mag, n), {"in": (s1, a)}, {"mag": d_mag}, dtypes={"mag": F32})
        assert orc.rel_l2(gg["mag"].view(F32), np.abs(a.astype(np.complex128))) < 1e-6
        ph, mg = _randf((n,), 3), np.abs(_randf((n,), 4))
        d_ph, d_mg, d_o = guarded(ctx, ph), guarded(ctx, mg), bufs["slc1_phase"]
        gk = _clean(ctx, lambda: ctx.mask_phase(d_ph, d_mg, n, 0.5, d_o), {"phase": (d_ph, ph), "mag": (d_mg, mg)}, {"out": d_o},
                    dtypes={"out": F32})
        assert np.array_equal(gk["out"].view(F32), np.where(mg > np.float32(0.5), ph, np.float32(0)))
        ctx.mask_phase(d_ph, d_mg, n, 0.5, d_ph)                     # d_out == d_phase
        ctx.sync()
        _zones_clean(d_ph, d_mg)
        assert np.array_equal(d_ph.download(), gk["out"])
        d_ph.upload(ph)
        ctx.ati_dpca(s1, s2, n, 0.0, {k: bufs[k] for k in ATI_REQ}, want_stats=False)      # sets the max the frac form reads
        gf = _clean(ctx, lambda: ctx.mask_phase_frac(d_ph, d_mg, n, 0.05, d_o), {"phase": (d_ph, ph), "mag": (d_mg, mg)}, {"out": d_o},
                    dtypes={"out": F32})["out"].view(F32)
        thr = 0.05 * ctx.ati_stats()[0]                              # sar_ati_dcpa_sim_csa.py:447-449 with max|slc1| of that launch
        keepm, drop = mg > thr * (1 + 1e-6), mg < thr * (1 - 1e-6)       # within fp32 rounding of the threshold: either way
        assert np.array_equal(gf[keepm], ph[keepm]) and not gf[drop].any()
        assert keepm.any() and drop.any() or n < 64                  # the mask does something
        # reductions: max_abs folds into *d_max, power_stats returns host doubles; a NaN read past the input would show in both
        d_m = GuardedBuffer(ctx, 4).zero()
        ctx.max_abs(d_mg, n, d_m)
        ctx.max_abs(d_ph, n, d_m)
        ctx.sync()
        assert d_m.download(F32)[0] == max(np.abs(ph).max(), mg.max())
        _zones_clean(d_m, d_mg, d_ph)
        assert np.array_equal(d_ph.download(F32), ph) and np.array_equal(d_mg.download(F32), mg)
        pmax, pmean = noise.power_stats(s1, n, ctx)
        p = np.abs(a.astype(np.complex128)) ** 2
        assert np.isfinite([pmax, pmean]).all() and abs(pmax - p.max()) <= 1e-6 * p.max() and abs(pmean - p.mean()) <= 1e-6 * p.mean()
        assert np.array_equal(s1.download(np.complex64), a)
        _zones_clean(s1)
        # noise: fill (an output), add_ocean_noise / _rel (in place: same bits twice, finite, zones clean)
        d_n = bufs["ati_interf"]
        _clean(ctx, lambda: ctx.fill_noise(d_n, n, 42), {}, {"noise": d_n}, dtypes={"noise": F32})
        for fn in (lambda: noise.add_noise_dev(d_n, n, 1.0, 10.0, seed=5, ctx=ctx), lambda: noise.add_noise_rel_dev(d_n, n, 10.0, seed=5, ctx=ctx),
                   lambda: noise.add_noise_rel_dev(d_n, n, 10.0, seed=5, ref="mean", ctx=ctx)):
            res = []
            for _ in range(2):
                d_n.upload(a)
                fn()
                ctx.sync()
                _zones_clean(d_n)
                res.append(d_n.download(F32))
            assert np.array_equal(res[0], res[1]) and np.isfinite(res[0]).all() and not np.array_equal(res[0], a.view(F32))
        _release(d_ph, d_mg, d_m)
    finally:
        _release(s1, s2, d_slot, *bufs.values())


# ---- corner turn, multilook, strided copies --------------------------------------------------------------------------------------
def corner_turn(sx, ctx, orc, rows, cols):
    z = zone_bytes(max(rows, cols) * 8)
    x = _rand((rows, cols), rows + cols)
    d_in, d_out = GuardedBuffer(ctx, x.nbytes, z), GuardedBuffer(ctx, x.nbytes, z)
    try:
        g = _clean(ctx, lambda: ctx.corner_turn(d_in, d_out, rows, cols), {"in": (d_in, x)}, {"out": d_out})
        assert np.array_equal(g["out"].view(np.complex64).reshape(cols, rows), x.T)           # moves bits only
    finally:
        _release(d_in, d_out)


def multilook(sx, ctx, orc, rows, cols, looks):
    z = zone_bytes(cols * 8)
    x = _rand((rows, cols), rows * cols + looks)
    d_in, d_out = GuardedBuffer(ctx, x.nbytes, z), GuardedBuffer(ctx, (rows // looks) * (cols // looks) * 4, z)
    try:
        g = _clean(ctx, lambda: ctx.multilook(d_in, d_out, rows, cols, looks), {"in": (d_in, x)}, {"out": d_out}, dtypes={"out": F32})
        ref = (np.abs(x.astype(np.complex128)) ** 2).reshape(rows // looks, looks, cols // looks, looks).mean(axis=(1, 3))
        assert orc.rel_l2(g["out"].view(F32).reshape(ref.shape), ref) < 1e-6                   # test_corner_turn_multilook_noise's bar
    finally:
        _release(d_in, d_out)


def memcpy2d(sx, ctx, orc, rows, cols, br, bc):
    """A block that ends at the last element of the image: nothing lands behind it, the rest of the image is not touched."""
    from sarx.engine import download_block, upload_block
    img = GuardedBuffer(ctx, rows * cols * 8, zone_bytes(cols * 8)).poison()
    blk = _rand((br, bc), 5)
    try:
        upload_block(ctx, img.ptr, cols, rows - br, cols - bc, blk)
        _zones_clean(img)
        full = img.download(np.complex64, (rows, cols))
        assert np.array_equal(full[rows - br:, cols - bc:], blk)
        rest = np.ones((rows, cols), bool)
        rest[rows - br:, cols - bc:] = False
        assert (full.view(np.uint8).reshape(rows, cols, 8)[rest] == 0xFF).all()
        assert np.array_equal(download_block(ctx, img.ptr, cols, rows - br, br, cols - bc, bc), blk)
        _zones_clean(img)
    finally:
        img.release()


# ---- range-Doppler focus ---------------------------------------------------------------------------------------------------
def rda(sx, ctx, orc, n_r, n_p, parity=True):
    from oracle import rda_oracle
    from sarx.rda import RdaPlan
    z = zone_bytes(n_r * 8)
    if parity:
        phist, args = rda_oracle.rda_scene(n_r, n_p, seed=5 * n_r + n_p)
    else:
        phist = _rand((n_r, n_p), n_r + n_p)
        k = orc.scaled_radar(n_p, n_r, chirp_fill=0.3)
        args = (k["Lambda"], k["T_p"], k["Kr"], k["FS"], k["PRF"], k["V_eff"], k["R0"])
    x = np.ascontiguousarray(phist.T)                                     # pulse-major memory
    plan = RdaPlan(ctx, n_r, n_p, _ffi.RadarParams(*args, 0.0))
    d_in = GuardedBuffer(ctx, x.nbytes, z)
    d_mag = GuardedBuffer(ctx, n_p * n_r * 4, z)
    maps = {k: GuardedBuffer(ctx, x.nbytes, z) for k in ("compressed", "doppler", "rcmc", "filtered")}
    try:
        outs = dict(maps, mag=d_mag)
        call2 = lambda: _ffi.check(ctx.lib.sarx_rda_focus_dev2(plan.h, d_in.ptr, d_mag.ptr, *(maps[k].ptr for k in maps)), ctx.h)
        g = _clean(ctx, call2, {"phist": (d_in, x)}, outs, dtypes={k: F32 for k in outs})
        three = {k: outs[k] for k in ("mag", "compressed", "doppler", "rcmc")}
        maps["filtered"].poison()
        call1 = lambda: _ffi.check(ctx.lib.sarx_rda_focus_dev(plan.h, d_in.ptr, d_mag.ptr, *(maps[k].ptr for k in ("compressed", "doppler", "rcmc"))), ctx.h)
        g1 = _clean(ctx, call1, {"phist": (d_in, x)}, three, dtypes={k: F32 for k in three})
        for k in three:
            assert np.array_equal(g1[k], g[k]), k
        assert (maps["filtered"].download() == 0xFF).all()       # poisoned by the run above and not requested since
        lean = lambda: _ffi.check(ctx.lib.sarx_rda_focus_dev(plan.h, d_in.ptr, d_mag.ptr, None, None, None), ctx.h)
        g0 = _clean(ctx, lean, {"phist": (d_in, x)}, {"mag": d_mag}, dtypes={"mag": F32})
        assert np.array_equal(g0["mag"], g["mag"])
        if parity:
            ref = rda_oracle.sar_focus_rda(phist, *args, variant="vehicle")
            for name, i in (("mag", 0), ("compressed", 3), ("doppler", 4), ("rcmc", 5), ("filtered", 6)):
                want = np.asarray(ref[i])
                got = g[name].view(F32 if name == "mag" else np.complex64).reshape(n_p, n_r)
                want = want if i == 0 else want.T                    # the complex maps come back [ranges x pulses]
                if np.linalg.norm(want) > 0:
                    err = orc.rel_l2(got, want)
                    print(f"rda {n_r}x{n_p} {name}: rel-L2 {err:.2e}")
                    assert err < TOL, (name, err)
    finally:
        plan.close()
        _release(d_in, d_mag, *maps.values())


# ---- echo synthesis --------------------------------------------------------------------------------------------------------
def _spotlight_numpy(tgt, vel, rcs, t_pulse, tx, velp, tf, c, fc, kr, t_p, l_ant, lam):
    """oracle/tdbp_oracle.py:run_physics_spotlight's arithmetic (sar_batch_sim.py:127-150) on a fast-time grid of the caller's."""
    t, ps, vs = t_pulse[:, None, None], tx[:, None, :], velp[:, None, :]
    p_tgt = tgt[None] + vel[None, None, :] * t
    d_tx_v = p_tgt - ps
    d_tx = np.linalg.norm(d_tx_v, axis=2)
    d_rx = np.linalg.norm(p_tgt - (ps + vs * (2 * d_tx / c)[:, :, None]), axis=2)
    tau = (d_tx + d_rx) / c
    look = -ps / np.linalg.norm(ps, axis=2, keepdims=True)
    ang = np.arccos(np.clip(np.sum(look * d_tx_v / d_tx[:, :, None], axis=2), -1, 1))
    x = np.pi * l_ant * np.sin(ang) / lam
    gain = np.ones_like(x)
    m = np.abs(x) > 1e-6
    gain[m] = (np.sin(x[m]) / x[m]) ** 2
    t_loc = tf[None, None, :] - tau[:, :, None]
    ph = np.pi * kr * t_loc ** 2 - 2 * np.pi * fc * tau[:, :, None]
    return np.sum((rcs[None, :] * gain)[:, :, None] * np.exp(1j * ph) * (np.abs(t_loc) <= t_p / 2), axis=1)


def echo(sx, ctx, orc, n_p, n_t, n_s):
    """Geometry launch of each model, then the sample launch on its table, against the NumPy signal models of oracle/ (5e-6, the
    bar of test_many_targets_and_focus_chain; 1e-4 for the spotlight model as test_spotlight_echo_golden).  The targets sit within
    40 m of the scene centre and the fast-time window is centred on the pulse, so the gate is open (asserted); at 129 samples
    the window is longer than the pulse and the gate closes inside it."""
    r = np.random.default_rng(n_p * 1000 + n_t * 10 + n_s)
    c_light, fc, t_p, fs = orc.C_LIGHT, 9.6e9, 2e-6, 60e6
    kr = 50e6 / t_p
    tgt = r.uniform(-40, 40, (n_t, 3))
    vel = r.uniform(-10, 10, 3)
    t_pulse = (np.arange(n_p) - n_p / 2) / 1000.0
    tx = np.stack([np.full(n_p, -5e5), 7000.0 * t_pulse, np.full(n_p, 5e5)], axis=1)
    velp = np.tile([0.0, 7000.0, 0.0], (n_p, 1))
    rxp = tx + velp / 7000.0 * 5.0                                   # receiver 5 m ahead along the velocity (echo_bistatic's rule)
    rcs = r.uniform(1, 50, n_t)
    amp = np.sqrt(rcs).astype(F32)
    targets = [{"position": p, "rcs": q} for p, q in zip(tgt, rcs)]
    tau0 = 2 * np.linalg.norm(tx[n_p // 2]) / c_light
    grid = np.linspace(0, n_s / fs, n_s)                             # the oracles' fast-time grid
    t0 = tau0 + t_p / 2 - n_s / fs / 2                               # models 0, 1: u = t - tau - Tp/2 runs through 0 mid-window
    t0_spot = tau0 - n_s / fs / 2                                    # model 2: u = t - tau
    l_ant, lam = 1.0, c_light / fc
    host = {"tgt": tgt, "vel": vel, "t": t_pulse, "tx": tx, "rx": rxp, "velp": velp, "rcs": rcs, "amp": amp, "tf": t0 + grid,
            "tf_spot": t0_spot + grid}
    d = {k: guarded(ctx, v) for k, v in host.items()}
    tab, apt = GuardedBuffer(ctx, n_p * n_t * 16), GuardedBuffer(ctx, n_p * n_t * 4)
    raw = GuardedBuffer(ctx, n_p * n_s * 8, zone_bytes(n_s * 8))
    geo = lambda model, v, t, aux, rc, ap: _ffi.check(ctx.lib.sarx_echo_geometry_dev(
        ctx.h, model, n_p, n_t, d["tgt"].ptr, v, t, d["tx"].ptr, aux, rc, c_light, fc, l_ant, lam, tab.ptr, ap), ctx.h)
    synth = lambda acc: _ffi.check(ctx.lib.sarx_echo_synth_dev(ctx.h, tab.ptr, d["amp"].ptr, d["tf"].ptr, n_p, n_t, n_s, kr, t_p, raw.ptr, acc), ctx.h)
    spot = lambda: _ffi.check(ctx.lib.sarx_echo_spotlight_dev(ctx.h, tab.ptr, apt.ptr, d["tf_spot"].ptr, n_p, n_t, n_s, kr, t_p, raw.ptr), ctx.h)
    ins = lambda *ks: {k: (d[k], host[k]) for k in ks}
    mono = lambda **kw: orc.echo_monostatic(targets, tx, n_s, fs, t0, fc, kr, t_p, **kw)
    models = (
        ("monostatic", lambda: geo(0, None, None, None, None, None), ("tgt", "tx"), mono, 5e-6),
        ("moving", lambda: geo(0, d["vel"].ptr, d["t"].ptr, None, None, None), ("tgt", "tx", "vel", "t"),
         lambda: mono(t_vec=t_pulse, vel_target=vel), 5e-6),
        ("bistatic", lambda: geo(1, d["vel"].ptr, d["t"].ptr, d["rx"].ptr, None, None), ("tgt", "tx", "vel", "t", "rx"),
         lambda: orc.echo_bistatic(targets, t_pulse, tx, velp, 5.0, vel, n_s, fs, t0, fc, kr, t_p), 5e-6),
        ("spotlight", lambda: geo(2, d["vel"].ptr, d["t"].ptr, d["velp"].ptr, d["rcs"].ptr, apt.ptr), ("tgt", "tx", "vel", "t", "velp", "rcs"),
         lambda: _spotlight_numpy(tgt, vel, rcs, t_pulse, tx, velp, host["tf_spot"], c_light, fc, kr, t_p, l_ant, lam), 1e-4))
    try:
        apt.poison()
        for name, call, used, oracle, bar in models:
            outs = {"tab": tab, "apt": apt} if name == "spotlight" else {"tab": tab}
            g = _clean(ctx, call, ins(*used), outs, dtypes={"tab": F64, "apt": F32})
            if name != "spotlight":
                assert (apt.download() == 0xFF).all()                # the spotlight model comes last: not written before it
            h_tab = g["tab"].copy()
            if name == "spotlight":
                h_apt = g["apt"].copy()
                g1 = _clean(ctx, spot, {"tab": (tab, h_tab), "tf": (d["tf_spot"], host["tf_spot"]), "apt": (apt, h_apt)}, {"raw": raw},
                            dtypes={"raw": F32})
            else:
                tabs = {"tab": (tab, h_tab), "tf": (d["tf"], host["tf"]), "amp": (d["amp"], amp)}
                g1 = _clean(ctx, lambda: synth(0), tabs, {"raw": raw}, dtypes={"raw": F32})
            got, ref = g1["raw"].view(np.complex64).reshape(n_p, n_s), oracle()
            assert np.count_nonzero(got) > 0 and np.count_nonzero(got) >= 0.5 * np.count_nonzero(ref), "the pulse gate is closed"
            err = orc.rel_l2(got, ref)
            print(f"echo {name} {n_p}p {n_t}t {n_s}s: rel-L2 {err:.2e}, {np.count_nonzero(got)} of {got.size} samples inside a pulse")
            assert err < bar, (name, err)
            if name == "bistatic":                                   # accumulate != 0 adds to d_raw
                raw.zero()
                synth(1)
                synth(1)
                ctx.sync()
                _zones_clean(raw, tab, d["amp"], d["tf"])
                once = g1["raw"].view(F32)
                assert np.array_equal(raw.download(F32), once + once) and once.any()
    finally:
        _release(tab, apt, raw, *d.values())


# ---- time-domain back-projection -------------------------------------------------------------------------------------------------
def tdbp(sx, ctx, orc, n_p, nx, ny, native=False, tile=True, mp=None):
    """tile=False forces the exact per-pixel kernel (SARX_TDBP_TILE=0, read at every focus).  tile=True allows the 16 x 16 tile
    expansion, which the library takes only for nx, ny >= 2 and metre-sized pixels: the native 90 x 70 case shows that it did by
    comparing with the exact kernel (different bits, rel-L2 < 2e-6: test_tile_expansion_equals_exact_kernel); the small shapes
    run the exact kernel either way."""
    from oracle import tdbp_oracle as tb
    k = tb.batch_constants() if native else tb.scaled_constants()
    sc = tb.tdbp_scene(n_pulses=n_p, seed=21 + n_p, k=k, swath=90.0 if native else 400.0, n_targets=4)
    rawh = sc["raw"].astype(np.complex64)
    n_s = sc["num_samples"]
    if not tile:
        mp.setenv("SARX_TDBP_TILE", "0")
    plan = sx.TdbpPlan(ctx, n_p, n_s, nx, ny, k)
    d_raw = guarded(ctx, rawh, zone_bytes(n_s * 8))
    d_img = GuardedBuffer(ctx, nx * ny * 16, zone_bytes(nx * 16))
    try:
        # TdbpPlan.focus takes its device-in / device-out path for a DeviceBuffer only: the C call is made here
        call = lambda: _ffi.check(ctx.lib.sarx_tdbp_focus_dev(
            plan.h, d_raw.ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(sc["t_start"]), vf.ctypes.data, float(sc["swath"]),
            d_img.ptr), ctx.h)
        pos, vel = np.ascontiguousarray(sc["pos"], dtype=F64), np.ascontiguousarray(sc["vel"], dtype=F64)
        tp, vf = np.ascontiguousarray(sc["t_vec"], dtype=F64), np.ascontiguousarray(sc["v_tgt"], dtype=F64)
        g = _clean(ctx, call, {"raw": (d_raw, rawh)}, {"image": d_img}, dtypes={"image": F64})
        ref = tb.tdbp(rawh, sc["pos"], sc["vel"], sc["t_start"], n_s, sc["v_tgt"], sc["t_vec"], sc["swath"], nx, ny, k)
        err = orc.rel_l2(g["image"].view(np.complex128).reshape(ny, nx), ref)
        print(f"tdbp {n_p} pulses {nx}x{ny} tile expansion {'allowed' if tile else 'off'}: rel-L2 {err:.2e}")
        assert err < TOL, err
        if native and tile:
            mp.setenv("SARX_TDBP_TILE", "0")
            call()
            ctx.sync()
            mp.delenv("SARX_TDBP_TILE")
            _zones_clean(d_raw, d_img)
            exact = d_img.download(np.complex128)
            tiled = g["image"].view(np.complex128)
            assert not np.array_equal(tiled, exact), "the tile-expansion kernel did not run"
            assert orc.rel_l2(tiled, exact) < 2e-6
    finally:
        if not tile:
            mp.delenv("SARX_TDBP_TILE")
        plan.close()
        _release(d_raw, d_img)


# ---- GMTI detection -----------------------------------------------------------------------------------------------------------
def _gmti_planes(n_az, n_rg, seed):
    rng = np.random.default_rng(seed)
    m = np.sqrt(rng.exponential(1.0, (n_az, n_rg))).astype(F32)
    k = max(6, n_az * n_rg // 1500)
    ii, jj = rng.integers(0, n_az, k), rng.integers(0, n_rg, k)
    m[ii, jj] = np.sqrt(10.0 ** rng.uniform(2.0, 6.0, k)).astype(F32)
    m[0, 0] = m[-1, -1] = m[0, -1] = 1e3
    return m, _rand((n_az, n_rg), seed + 1), _rand((n_az, n_rg), seed + 2)


def gmti(sx, ctx, orc, n_az, n_rg, outer):
    """outer = (guard_az + train_az, guard_rg + train_rg): the halo that picks the <HA, HR> instantiation."""
    from sarx import gmti as G
    guard = (1, 1)
    train = (outer[0] - 1, outer[1] - 1)
    m, a, b = _gmti_planes(n_az, n_rg, n_az + 7 * n_rg + outer[0] * 100 + outer[1])
    z = zone_bytes(n_rg * 8)
    d_m, d_1, d_2 = guarded(ctx, m, z), guarded(ctx, a, z), guarded(ctx, b, z)
    ins = {"dpca_mag": (d_m, m), "slc1": (d_1, a), "slc2": (d_2, b)}
    o = gref.cfar(m, guard, train, pfa=1e-3)
    count = len(o["cells"])
    slots = []
    try:
        for cap in sorted({max(count, 1) + 7, max(count, 1), max(count - 1, 1), 1}, reverse=True):
            p = G.GmtiParams(guard, train, 1e-3, None, cap)
            slot = GuardedBuffer(ctx, p.slot_bytes())
            slots.append(slot)
            assert slot.nbytes == 16 + 48 * cap

            def promised(bytes_, cap=cap):
                n = int(bytes_[:4].view("<u4")[0])
                mask = np.zeros(len(bytes_), bool)
                mask[:16 + 48 * min(n, cap)] = True
                if n > cap:                                          # overflowed: which cells made it is not defined; the list still ends at cap
                    mask[16:] = False
                    return {"promised": mask, "scratch": ~mask}
                return mask
            g = _clean(ctx, lambda: G.enqueue(ctx, d_m.ptr, d_1.ptr, d_2.ptr, n_az, n_rg, p, 0.4, slot.ptr), ins, {"slot": slot},
                       promised={"slot": promised})
            n, overflow = (int(v) for v in g["slot"][:8].view("<u4"))
            assert overflow == (1 if n > cap else 0)
            if not overflow:
                rep = g["slot"][16:16 + 48 * n].view(G.REPORT_DTYPE)
                cells = list(zip(rep["i"].tolist(), rep["j"].tolist()))
                assert cells == sorted(cells)
                missing, extra = gref.compare(cells, o)
                assert not missing and not extra, (missing[:5], extra[:5], n, count)
                assert np.isfinite(rep["power"]).all() and np.isfinite(rep["interf_re"]).all() and np.isfinite(rep["mag2"]).all()
                want = gref.interferogram(a, b, cells, 0.4)
                scale = np.array([np.sum(np.abs(a[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2]) * np.abs(b[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2]))
                                  for i, j in cells])
                assert np.all(np.abs(rep["interf_re"] + 1j * rep["interf_im"] - want) <= 1e-6 * scale)    # test_parity_on_synthetic_planes' bar
    finally:
        _release(d_m, d_1, d_2, *slots)


# ---- GMTI refocus -------------------------------------------------------------------------------------------------------------
def refocus(sx, ctx, orc, L, W, source):
    from sarx import gmti as G, refocus as R
    lam, v, prf, r0, dr = 0.031, 200.0, 1000.0, 5000.0, 1.0
    n_az, n_rg = 700, 203
    pos = np.array([(0, 100), (n_az - 1, 60), (350, 0), (200, n_rg - 1), (0, 0), (n_az - 1, n_rg - 1)], np.int64)
    p = sx.RefocusParams(chip=(L, W), v_along=(-30.0, 30.0), n_hyp=13, source=source, want_curves=True, want_chips=True)
    a, b = _rand((n_az, n_rg), L + W), _rand((n_az, n_rg), L + W + 1)
    cp = p.c_params(lam, v, prf, r0, dr, 0.3)
    cap = len(pos) + 2
    z = zone_bytes(n_rg * 8)
    d_1, d_2 = guarded(ctx, a, z), guarded(ctx, b, z)
    rec, cur, chips = GuardedBuffer(ctx, cap * 48), GuardedBuffer(ctx, cap * 13 * 4), GuardedBuffer(ctx, cap * L * W * 8)
    outs = {"records": rec, "curves": cur, "chips": chips}
    slots = []
    try:
        for n, overflow in ((len(pos), 0), (0, 0), (cap + 1, 1)):
            raw = np.zeros(16 + cap * 48, np.uint8)
            raw[:8].view("<u4")[:] = [n, overflow]
            rp = raw[16:].view(G.REPORT_DTYPE)
            rp["i"][:len(pos)], rp["j"][:len(pos)] = pos[:, 0], pos[:, 1]
            slot = guarded(ctx, raw)
            slots.append(slot)
            k = 0 if overflow else n                                 # an overflowed slot: nothing at all is written
            g = _clean(ctx, lambda: R.enqueue(ctx, d_1.ptr, d_2.ptr if source == "dpca" else None, n_az, n_rg, cp, slot.ptr, cap,
                                              rec.ptr, cur.ptr, chips.ptr),
                       {"slc1": (d_1, a), "slc2": (d_2, b), "slot": (slot, raw)}, outs,
                       promised={"records": k * 48, "curves": k * 13 * 4, "chips": k * L * W * 8}, dtypes={"curves": F32, "chips": F32})
            if k:
                want = rref.refocus(a, b if source == "dpca" else None, pos, L, W, p.speeds(v), lam, v, prf, r0, dr, source, 0.3)
                r = g["records"][:k * 48].view(R.RECORD_DTYPE)
                curves = g["curves"][:k * 13 * 4].view(F32).reshape(k, 13)
                for q, w in enumerate(want):
                    assert r["i0"][q] == w["i0"] == min(max(pos[q][0] - L // 2, 0), n_az - L)
                    np.testing.assert_allclose(curves[q], w["curve"], rtol=1e-4, err_msg=f"report {q}")     # test_gpu_refocus.py's bar
    finally:
        _release(d_1, d_2, rec, cur, chips, *slots)


# ---- single-rank collectives -----------------------------------------------------------------------------------------------------
def collectives(sx, ctx, orc):
    from sarx.batch import RcclStackComm
    x = _randf((4097,), 9)
    d_s, d_r = guarded(ctx, x), GuardedBuffer(ctx, x.nbytes)
    comm = RcclStackComm(ctx, 1, 0)
    try:
        def gather():
            comm.all_gather_dev(d_s, d_r, x.nbytes)
            comm.finish()
        g = _clean(ctx, gather, {"send": (d_s, x)}, {"recv": d_r}, dtypes={"recv": F32})
        assert np.array_equal(g["recv"].view(F32), x)
        ctx.allreduce_max(d_s, x.size)                               # in place; one rank: the identity
        comm.finish()
        ctx.sync()
        _zones_clean(d_s)
        assert np.array_equal(d_s.download(F32), x)
    finally:
        ctx.lib.sarx_comm_destroy(ctx.h)
        _release(d_s, d_r)


# ---- offset views: a pointer 8 bytes past a 16-byte boundary, as DeviceArray.rows(1, n) hands out for even n_rg ------------------
def offset_views(sx, ctx, orc, what, n_az, n_rg):
    from sarx.rda import RdaPlan
    x = _rand((n_az, n_rg), n_az + n_rg)
    px = n_az * n_rg
    z = zone_bytes(max(n_az, n_rg) * 8)
    close = lambda: None
    if what == "focus":
        plan = sx.CsaPlan(ctx, n_az, n_rg, *orc.focus_args(orc.scaled_radar(max(n_az, 16), max(n_rg, 16))), flags=_ffi.FUSE_RANGE)
        out_bytes, call, close = px * 8, lambda i, o: plan.focus_dev(i, o), plan.close
    elif what.startswith("pass"):
        plan = sx.CsaPlan(ctx, n_az, n_rg, *orc.focus_args(orc.scaled_radar(n_az, n_rg)))
        out_bytes, call, close = px * 8, lambda i, o, pid=int(what[4:]): plan.run_pass(pid, i, o), plan.close
    elif what == "rda":
        k = orc.scaled_radar(n_az, n_rg, chirp_fill=0.3)
        plan = RdaPlan(ctx, n_rg, n_az, _ffi.RadarParams(k["Lambda"], k["T_p"], k["Kr"], k["FS"], k["PRF"], k["V_eff"], k["R0"], 0.0))
        out_bytes, close = px * 4, plan.close
        call = lambda i, o: _ffi.check(ctx.lib.sarx_rda_focus_dev(plan.h, i.ptr, o.ptr, None, None, None), ctx.h)
    elif what == "magnitude":
        out_bytes, call = px * 4, lambda i, o: ctx.magnitude(i, o, px)
    elif what == "corner_turn":
        out_bytes, call = px * 8, lambda i, o: ctx.corner_turn(i, o, n_az, n_rg)
    elif what == "multilook":
        out_bytes, call = px * 4, lambda i, o: ctx.multilook(i, o, n_az, n_rg - n_rg % 2, 1)
        x = np.ascontiguousarray(x[:, :n_rg - n_rg % 2])
        out_bytes = x.size * 4
    elif what == "mask_phase":
        x = _randf((2 * px,), 3)
        mg = guarded(ctx, np.abs(_randf((2 * px,), 4)))
        out_bytes, call, close = 2 * px * 4, lambda i, o: ctx.mask_phase(i, mg, 2 * px, 0.5, o), mg.release
    elif what == "mask_phase_frac":
        x = _randf((2 * px,), 3)
        mg = guarded(ctx, np.abs(_randf((2 * px,), 4)))
        s1 = guarded(ctx, _rand((px,), 5))
        tmp = {k: GuardedBuffer(ctx, px * 4) for k in ATI_REQ}
        ctx.ati_dpca(s1, s1, px, 0.0, tmp, want_stats=False)             # leaves max|slc1| on the device for the frac form
        ctx.sync()
        _release(s1, *tmp.values())
        out_bytes, call, close = 2 * px * 4, lambda i, o: ctx.mask_phase_frac(i, mg, 2 * px, 0.05, o), mg.release
    bufs = []
    try:
        res = {}
        for name, off_in, off_out in (("aligned", 0, 0), ("input + 8", 8, 0), ("output + 8", 0, 8)):
            d_in = GuardedBuffer(ctx, x.nbytes, z, offset=off_in)
            d_out = GuardedBuffer(ctx, out_bytes, z, offset=off_out)
            bufs += [d_in, d_out]
            res[name] = _clean(ctx, lambda: call(d_in, d_out), {"in": (d_in, x)}, {"out": d_out}, dtypes={"out": F32})["out"]
        assert np.array_equal(res["input + 8"], res["aligned"]), "input at offset 8"
        assert np.array_equal(res["output + 8"], res["aligned"]), "output at offset 8"
    finally:
        close()
        _release(*bufs)


def offset_reductions_and_noise(sx, ctx, orc, n):
    """The product kernels without a separate output plane, with the buffer 8 bytes (max_abs, whose scalar head runs up to the first
    16-byte boundary: also 4) past the aligned position, the zones' NaN right beside it: the same values as aligned."""
    from sarx import noise
    x, c = _randf((n,), n), _rand((n,), n + 1)
    bufs = []

    def at(arr, off, nbytes=None):
        b = GuardedBuffer(ctx, arr.nbytes if nbytes is None else nbytes, offset=off)
        bufs.append(b)
        return b.upload(arr)
    try:
        for pos in (0, n // 2, n - 1):                               # the extreme value in the head, the body and the tail
            y = x.copy()
            y[pos] = -77.0
            for off_x, off_m in ((0, 0), (4, 0), (8, 0), (12, 0), (0, 4), (0, 8), (8, 8)):
                d_x, d_m = at(y, off_x), at(np.zeros(1, F32), off_m)
                ctx.max_abs(d_x, n, d_m)
                ctx.sync()
                assert d_m.download(F32)[0] == np.float32(77.0), (pos, off_x, off_m)
                _zones_clean(d_x, d_m)
                assert np.array_equal(d_x.download(F32), y)
            _release(*bufs)
            del bufs[:]
        stats = [noise.power_stats(at(c, off), n, ctx) for off in (0, 8)]
        assert stats[0] == stats[1] and np.isfinite(stats[0]).all()
        _zones_clean(*bufs)
        fills = []
        for off in (0, 8):
            d = GuardedBuffer(ctx, n * 8, offset=off)
            bufs.append(d)
            fills.append(_clean(ctx, lambda: ctx.fill_noise(d, n, 42), {}, {"noise": d}, dtypes={"noise": F32})["noise"])
        assert np.array_equal(fills[0], fills[1])
        for fn in (lambda d: noise.add_noise_dev(d, n, 1.0, 10.0, seed=5, ctx=ctx), lambda d: noise.add_noise_rel_dev(d, n, 10.0, seed=5, ctx=ctx),
                   lambda d: noise.add_noise_rel_dev(d, n, 10.0, seed=5, ref="mean", ctx=ctx)):
            res = []
            for off in (0, 8):
                d = at(c, off)
                fn(d)
                ctx.sync()
                _zones_clean(d)
                res.append(d.download(F32))
            assert np.array_equal(res[0], res[1]) and np.isfinite(res[0]).all()
    finally:
        _release(*bufs)


def offset_ati(sx, ctx, orc, n):
    """include/sarx.h states 16-byte alignment for the ATI / DPCA buffers and the entry points enforce it: SARX_ERR_INVALID, nothing
    launched, nothing written."""
    x = _rand((n,), n)
    s2 = guarded(ctx, x)
    outs = {k: GuardedBuffer(ctx, n * 4).poison() for k in ATI_REQ}
    d_slot = GuardedBuffer(ctx, 32768).zero()
    bufs = [s2, d_slot, *outs.values()]
    try:
        for off_in, off_out in ((8, 0), (0, 8)):
            s1 = GuardedBuffer(ctx, x.nbytes, offset=off_in).upload(x)
            o = dict(outs)
            if off_out:
                o["dpca_mag"] = GuardedBuffer(ctx, n * 4, offset=off_out).poison()
            bufs += [s1, o["dpca_mag"]]
            for call in (lambda: ctx.ati_dpca(s1, s2, n, 0.0, o, want_stats=False), lambda: ctx.ati_dpca_masked(s1, s2, n, 0.0, d_slot, 0.05, o)):
                with pytest.raises(sx.SarxError) as e:
                    call()
                assert e.value.code == -1 and "16-byte" in str(e.value)
            ctx.sync()
            _zones_clean(s1, s2, *o.values())
            assert all((b.download() == 0xFF).all() for b in o.values())
    finally:
        _release(*bufs)


E = "sarx_"
PASS, FOCUS = {E + "csa_pass"}, {E + "csa_focus_dev"}
PRODUCTS = {E + n for n in ("ati_dpca_dev", "ati_dpca_masked_dev", "magnitude_dev", "mask_phase_dev", "mask_phase_frac_dev",
                            "max_abs_f32_dev", "power_stats_dev", "fill_noise_c64", "add_ocean_noise_dev", "add_ocean_noise_rel_dev")}
ECHO = {E + n for n in ("echo_geometry_dev", "echo_synth_dev", "echo_spotlight_dev")}
GMTI = {E + "gmti_cfar_dev", E + "gmti_refine_dev"}
FUSE, RG_MAJOR = _ffi.FUSE_RANGE, _ffi.OUT_RG_MAJOR

# (id, entry points, family, arguments).  Outputs, inputs and the promised extents are stated in the family functions above.
CASES = []


def _add(cid, entry, fn, *args, **kw):
    CASES.append((cid, entry, fn, args, kw))


for _shape in ((16, 16), (64, 128)):                                       # no per-pass parity test has these two shapes
    _add("pass-%dx%d" % _shape, PASS, csa_pass, *_shape, (1, 2, 3, 4, 23, 100, 101), parity=True)
for _shape in ((256, 16), (16, 256), (2048, 512)):                         # az_w = 16 and 32 tiles; the four-step azimuth transform
    _add("pass-%dx%d" % _shape, PASS, csa_pass, *_shape, (1, 2, 3, 4, 23, 100, 101))
_add("pass-16x16384", PASS, csa_pass, 16, 16384, (12, 13, 2, 3, 23))
_add("pass-1024x16384", PASS, csa_pass, 1024, 16384, (12, 13, 2, 3, 23))   # every persistent workgroup walks several lines
_add("pass-1024x16384-192cus", PASS, csa_pass, 1024, 16384, (23,), range_cus=192)      # the benchmark's share: ragged last iteration
_add("pass-az-wave-16384x32-1wave", PASS, csa_pass, 16384, 32, (110, 111, 112, 113, 1, 4), flags=FUSE, az_waves=1)
_add("pass-az-wave-16384x64-1wave", PASS, csa_pass, 16384, 64, (110, 111, 112, 113, 1, 4), flags=FUSE, az_waves=1)
_add("pass-az-wave-16384x128-4waves", PASS, csa_pass, 16384, 128, (110, 111, 112, 113, 1, 4), flags=FUSE, az_waves=4)   # the default workgroup
for _shape, _par in (((64, 64), False), ((512, 1024), False), ((4096, 2048), False)):
    for _flags in (0, FUSE, RG_MAJOR):
        if _shape == (4096, 2048) and _flags == RG_MAJOR:
            continue                                                        # the largest shape once per route: fused and unfused
        _add("focus-%dx%d-flags%d" % (*_shape, _flags), FOCUS, focus, *_shape, flags=_flags)
_add("focus-512x1024-slab", FOCUS, focus, 512, 1024, flags=FUSE, slab=1)
_add("focus-4096x2048-slab", FOCUS, focus, 4096, 2048, flags=FUSE, slab=16)
for _shape in ((2, 2), (5, 7), (17, 17), (255, 257), (33, 1024), (2, 1000), (1000, 2)):
    _add("focus-general-%dx%d" % _shape, FOCUS, focus, *_shape, parity=_shape not in ((255, 257), (5, 7), (33, 1024)))
_add("focus-native-7199x13200", FOCUS, focus, 7199, 13200, flags=FUSE)
_EPI = FOCUS | {E + "csa_plan_set_look_slot", E + "csa_plan_set_max_slot", E + "csa_plan_set_ati", E + "ati_dpca_masked_dev"}
_add("epilogues-64x128", _EPI, epilogues, 64, 128, looks=(1, 4, 32), keep=False)
_add("epilogues-2048x512", _EPI, epilogues, 2048, 512, looks=(1, 4, 32), keep=True)
_add("epilogues-2048x512-scratch-image", _EPI, epilogues, 2048, 512, keep=False)
_add("epilogues-64x128-keep", _EPI, epilogues, 64, 128, keep=True)
_add("epilogues-native-7199x13200", _EPI, epilogues, 7199, 13200, keep=False)
_add("epilogues-native-7199x13200-keep", _EPI, epilogues, 7199, 13200, keep=True)      # the any-size route's own epilogue path writes slc2
for _n in (1, 63, 64, 65, 4097, 1_000_003):
    _add("products-n%d" % _n, PRODUCTS, products, _n)
_add("products-n2^25+4", PRODUCTS, products, (1 << 25) + 4, alone=False)    # the nontemporal switch of the ATI launch
for _shape in ((1, 1), (65, 3), (100, 77), (7199, 40), (64, 8192), (9000, 8200), (3, 65), (33, 31)):
    _add("corner-turn-%dx%d" % _shape, {E + "corner_turn_dev"}, corner_turn, *_shape)
for _r, _c, _l in ((1, 2, 1), (65, 4, 1), (100, 78, 1), (4, 8, 4), (100, 76, 4), (260, 1028, 4), (16, 32, 16), (48, 80, 16), (272, 1040, 16)):
    _add("multilook-%dx%d-L%d" % (_r, _c, _l), {E + "multilook_dev"}, multilook, _r, _c, _l)
_add("memcpy2d-last-block", {E + "memcpy2d_h2d", E + "memcpy2d_d2h"}, memcpy2d, 77, 203, 5, 9)
_RDA = {E + "rda_focus_dev", E + "rda_focus_dev2"}
for _shape in ((2, 2), (40, 3), (257, 101), (333, 256), (1024, 512)):
    _add("rda-%dx%d" % _shape, _RDA, rda, *_shape)
_add("rda-native-13200x7200", _RDA, rda, 13200, 7200, parity=False)
for _shape in ((1, 1, 1), (7, 3, 100), (65, 5, 129), (130, 2, 63)):
    _add("echo-%dp-%dt-%ds" % _shape, ECHO, echo, *_shape)
_TD = {E + "tdbp_focus_dev"}
for _shape in ((1, 1, 1), (5, 1, 7), (33, 17, 16)):
    _add("tdbp-%dp-%dx%d" % _shape, _TD, tdbp, *_shape)
_add("tdbp-64p-90x70-tile", _TD, tdbp, 64, 90, 70, native=True)
_add("tdbp-64p-90x70-exact", _TD, tdbp, 64, 90, 70, native=True, tile=False)
for _shape in ((33, 65), (96, 80), (1000, 777)):
    for _ha in (8, 16, 32):
        for _hr in (8, 16, 32):
            _add("gmti-%dx%d-H%d-%d" % (*_shape, _ha, _hr), GMTI, gmti, *_shape, (_ha, _hr))
for _L, _W, _src in ((256, 5, "dpca"), (256, 5, "slc1"), (512, 15, "dpca"), (512, 15, "slc1")):
    _add("refocus-L%d-W%d-%s" % (_L, _W, _src), {E + "refocus_dev"}, refocus, _L, _W, _src)
_add("collectives-single-rank", {E + "allgather_dev", E + "allreduce_max_dev"}, collectives)
for _what, _entry in (("focus", FOCUS), ("rda", {E + "rda_focus_dev"}), ("magnitude", {E + "magnitude_dev"}),
                      ("corner_turn", {E + "corner_turn_dev"}), ("multilook", {E + "multilook_dev"}), ("mask_phase", {E + "mask_phase_dev"}),
                      ("mask_phase_frac", {E + "mask_phase_frac_dev"})):
    for _shape in ((255, 257), (256, 256)):
        _add("offset8-%s-%dx%d" % (_what, *_shape), _entry, offset_views, _what, *_shape)
for _n in (255 * 257, 65536):
    _add("offset8-reductions-noise-n%d" % _n, {E + n for n in ("max_abs_f32_dev", "power_stats_dev", "fill_noise_c64", "add_ocean_noise_dev",
                                                              "add_ocean_noise_rel_dev")}, offset_reductions_and_noise, _n)
for _n in (255 * 257, 65536):
    _add("offset8-ati-n%d" % _n, {E + "ati_dpca_dev", E + "ati_dpca_masked_dev"}, offset_ati, _n)
for _pid in (1, 2, 3, 4, 23):
    _add("offset8-pass%d-256x256" % _pid, PASS, offset_views, "pass%d" % _pid, 256, 256)
_add("offset8-pass23-48x13200", PASS, offset_views, "pass23", 48, 13200)          # the any-size plans' per-pass entry: direct 13200 lines


def covered_entry_points():
    return set().union(*(c[1] for c in CASES))


@pytest.fixture(scope="module")
def sx():
    import sarx
    return sarx


@pytest.fixture(scope="module")
def ctx(sx):
    return sx.default_context()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_guard(sx, ctx, case, monkeypatch):
    from oracle import csa_oracle as orc
    _, _, fn, args, kw = case
    if "mp" in inspect.signature(fn).parameters:                # the families that set an environment switch for a plan
        kw = dict(kw, mp=monkeypatch)
    fn(sx, ctx, orc, *args, **kw)
