"""Every launch of the four-step azimuth transform (sarx_csa_pass ids 110-113: forward A, forward B, inverse A, inverse B) against
the complex128 step oracle of tests/_az_steps_numpy.py, at every four-step size, tile width, route and epilogue, on images a few
columns wide.  Each result is held by three bounds (accept()): whole-image and per-column relative L2 5e-6, worst row 1e-5, worst
element within 8 x the complex64 NumPy comparator's own worst element on the same input.  No row, column or element is left out.

The routes are chosen per plan from the environment (api_csa.hip: SARX_AZ_W, SARX_AZ_NT, SARX_AZ_IMPL, SARX_AZ_WAVES) or per call
(SARX_ATI_W), so monkeypatch around the plan's creation is enough.  Every check prints its figures (`pytest -s`): DESIGN section 2
holds the table.  Not covered here: the inverse split S <-> RA of slab mode on the device (no per-step entry point; the oracle
serves it, tests/test_az_steps.py) and the single-launch sizes n_az <= 128."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _az_steps_numpy as az  # noqa: E402
from oracle import csa_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = list(az.PLAN_SPLITS)
ENV_KEYS = ("SARX_AZ_W", "SARX_AZ_NT", "SARX_AZ_IMPL", "SARX_AZ_WAVES", "SARX_ATI_W", "SARX_SLAB_MIB")
MAX_REL = 2e-7          # the max slot against max |oracle|, as test_gpu_anysize.py holds it against the image


def _cases():
    c = []
    for n in SIZES:
        c.append((f"default-{n}x64", n, 64, {}))
        c.append((f"w16only-{n}x16", n, 16, {}))                        # n_rg = 16: width 16 is the only one, one column tile
        c.append((f"W16-{n}x64", n, 64, {"SARX_AZ_W": "16"}))
        c.append((f"W64-{n}x64", n, 64, {"SARX_AZ_W": "64"}))
    for n in (256, 2048, 8192):
        c.append((f"W64-{n}x256", n, 256, {"SARX_AZ_W": "64"}))          # several column tiles
    c.append(("W64-tile-16384x256", 16384, 256, {"SARX_AZ_W": "64", "SARX_AZ_IMPL": "0"}))   # the wave route ignores the width
    for n in (256, 2048, 8192, 16384):
        c.append((f"NT-{n}x64", n, 64, {"SARX_AZ_NT": "1"}))
    c.append(("NT-wave-16384x128", 16384, 128, {"SARX_AZ_NT": "1"}))
    c.append(("residues-8192x128", 8192, 128, {}))                       # 128 columns: the impulses hit every residue mod RA = 128
    c.append(("tile-16384x64", 16384, 64, {"SARX_AZ_IMPL": "0"}))
    c.append(("tile-16384x128", 16384, 128, {"SARX_AZ_IMPL": "0"}))
    c.append(("wave1-16384x32", 16384, 32, {"SARX_AZ_IMPL": "1", "SARX_AZ_WAVES": "1"}))
    c.append(("wave1-16384x64", 16384, 64, {"SARX_AZ_IMPL": "1", "SARX_AZ_WAVES": "1"}))
    c.append(("wave4-16384x128", 16384, 128, {}))                        # the default four waves: one workgroup per tile row ...
    c.append(("wave4-16384x256", 16384, 256, {}))                        # ... and two
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def sx():
    import sarx
    return sarx


@pytest.fixture(scope="module")
def ctx(sx):
    return sx.default_context()


def _args(n_az, n_rg):
    return orc.focus_args(orc.scaled_radar(n_az, n_rg))


@pytest.fixture(scope="module")
def plans(sx, ctx):
    made = {}

    def get(monkeypatch, n_az, n_rg, env):
        key = (n_az, n_rg, tuple(sorted(env.items())))
        if key not in made:
            for k in ENV_KEYS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            made[key] = sx.CsaPlan(ctx, n_az, n_rg, *_args(n_az, n_rg))
            for k in env:
                monkeypatch.delenv(k)
        return made[key]

    yield get
    for p in made.values():
        p.close()


_REF = {}


def _reference(n_az, n_rg, sid, name):
    """(input, complex128 oracle result, the complex64 comparator's worst element): computed once, shared, left unchanged"""
    key = (n_az, n_rg, sid, name)
    if key not in _REF:
        S = az.PLAN_SPLITS[n_az][0]
        x = az.INPUTS[name](n_az, n_rg)
        phi = az.phi1_table(n_az, n_rg, np.arange(n_rg), _args(n_az, n_rg)) if sid == az.FWD_B else None
        ref = az.run_step(sid, x, S, phi)
        cmp_elem = az.step_errors(az.run_step(sid, x, S, phi, dtype=np.complex64), ref)["elem"]
        x.setflags(write=False)
        ref.setflags(write=False)
        if n_rg > 64:                      # used by one or two cases each: not kept
            return x, ref, cmp_elem
        _REF[key] = (x, ref, cmp_elem)
    return _REF[key]


def _run(ctx, plan, sid, x, d_in, d_out):
    d_in.upload(x)
    plan.run_pass(sid, d_in, d_out)
    return d_out.download(np.complex64, x.shape)


@pytest.mark.parametrize("sid", az.STEP_IDS, ids=[az.STEP_NAMES[s] for s in az.STEP_IDS])
@pytest.mark.parametrize("label,n_az,n_rg,env", CASES, ids=[c[0] for c in CASES])
def test_step_against_the_oracle(sx, ctx, plans, monkeypatch, label, n_az, n_rg, env, sid):
    """One launch, three inputs, three bounds; id 113 with the max slot armed (the slot against max |oracle| to 2e-7).

    Found by this test: inverse step B of n_az = 16384 on az_tile_kernel<128> was 17.4 x the comparator on the impulses (5.85e-6 of
    the column's RMS against 3.37e-7) and 8.2-8.3 x on noise at 128 / 256 columns, every other bound holding: the 128-point tile's
    radix-8 stage multiplied by w^2 .. w^7 built from one hardware-evaluated w.  Each power is now evaluated on its own
    (fft_core.hpp, DIRECT_TW): 6.2 x, and 2.5 x instead of 6.0 x in its other three steps."""
    from sarx import _ffi
    plan = plans(monkeypatch, n_az, n_rg, env)
    nbytes = n_az * n_rg * 8
    d_in, d_out, d_max = ctx.alloc(nbytes), ctx.alloc(nbytes), ctx.alloc(_ffi.MAX_SLOT_BYTES)
    try:
        for name in az.INPUTS:
            x, ref, cmp_elem = _reference(n_az, n_rg, sid, name)
            if sid == az.INV_B:               # with the max slot armed: stale contents must not survive
                ctx.lib.sarx_memset(ctx.h, d_max.ptr, 0xFF, _ffi.MAX_SLOT_BYTES)
                plan.set_max_slot(d_max)
            ctx.lib.sarx_memset(ctx.h, d_out.ptr, 0xFF, nbytes)        # NaN everywhere: a row that is not written shows
            got = _run(ctx, plan, sid, x, d_in, d_out)
            e = az.step_errors(got, ref)
            print(f"AZSTEP {label} {az.STEP_NAMES[sid]} {name}: rel_l2 {e['rel_l2']:.3e} col_l2 {e['col_l2']:.3e} row {e['row']:.3e} "
                  f"row_n {e['row_n']:.3e} elem {e['elem']:.3e} cmp {cmp_elem:.3e} ratio {e['elem'] / max(cmp_elem, az.ELEM_FLOOR):.2f}")
            if sid == az.INV_B:
                plan.set_max_slot(None)
                shards = d_max.download(np.float32, (256, 32))
                want = float(np.abs(ref).max())
                print(f"AZSTEP {label} max_slot {name}: {(float(shards[:, 0].max()) - want) / want:+.3e}")
            az.accept(got, ref, cmp_elem, f"{label} {az.STEP_NAMES[sid]} {name}")
            if sid == az.INV_B:
                assert not shards[:, 1:].any()
                assert abs(float(shards[:, 0].max()) - want) <= MAX_REL * want, (float(shards[:, 0].max()), want)
    finally:
        plan.set_max_slot(None)
        for b in (d_in, d_out, d_max):
            b.release()


@pytest.mark.parametrize("n_rg,wave_env", [(64, {"SARX_AZ_IMPL": "1", "SARX_AZ_WAVES": "1"}), (128, {})], ids=["one_wave_x64", "four_waves_x128"])
def test_wave_and_tile_routes_differ_in_bits(sx, ctx, plans, monkeypatch, n_rg, wave_env):
    """Both routes are held by the oracle above; that they are two routes shows in the bits (another order of additions), which is
    the guard suite's proof that SARX_AZ_IMPL selected something."""
    n = 16384
    tile, wave = plans(monkeypatch, n, n_rg, {"SARX_AZ_IMPL": "0"}), plans(monkeypatch, n, n_rg, wave_env)
    d_in, d_out = ctx.alloc(n * n_rg * 8), ctx.alloc(n * n_rg * 8)
    try:
        x = az.INPUTS["noise"](n, n_rg)
        for sid in az.STEP_IDS:
            a, b = _run(ctx, tile, sid, x, d_in, d_out), _run(ctx, wave, sid, x, d_in, d_out)
            assert not np.array_equal(a, b), az.STEP_NAMES[sid]
            assert orc.rel_l2(a, b) < 1e-6
    finally:
        d_in.release(); d_out.release()


# ---- the epilogues that have no step id (look slot, ATI products), at forced widths, through PASS_AZ_IFFT ------------------------------
@pytest.mark.parametrize("n_az,n_rg", [(1024, 64), (2048, 256)])
@pytest.mark.parametrize("width", [16, 32, 64])
def test_look_slot_at_forced_widths(sx, ctx, plans, monkeypatch, n_az, n_rg, width):
    """AZ_EPI_SCALE_LOOK at tile widths 16, 32 and 64, looks 4 and 16, against the multilook of the oracle's image.  looks <= az_w is
    the plan's condition (sarx_csa_plan_set_look_slot), so 16 looks at width 16 are accepted and checked; 32 are refused there."""
    from sarx import _ffi
    plan = plans(monkeypatch, n_az, n_rg, {"SARX_AZ_W": str(width)})
    x = az.INPUTS["noise"](n_az, n_rg)
    img = orc.azimuth_ifft_cols(x)
    d_in, d_out = ctx.to_device(x), ctx.alloc(x.nbytes)
    try:
        for looks in (4, 16):
            nslot = (n_az // looks) * (n_rg // looks)
            d_slot = ctx.alloc(nslot * 4 + 64)
            ctx.lib.sarx_memset(ctx.h, d_slot.ptr, 0xFF, nslot * 4 + 64)
            plan.set_look_slot(looks, d_slot.ptr)
            plan.run_pass(_ffi.PASS_AZ_IFFT, d_in, d_out)
            plan.set_look_slot(looks, None)
            slot = d_slot.download(np.float32, (n_az // looks, n_rg // looks))
            guard = d_slot.download(np.uint8, (nslot * 4 + 64,))[nslot * 4:]
            d_slot.release()
            ref = (np.abs(img) ** 2).reshape(n_az // looks, looks, n_rg // looks, looks).mean(axis=(1, 3))
            err = np.linalg.norm(slot.astype(np.float64) - ref) / np.linalg.norm(ref)
            worst = np.abs(slot - ref).max() / np.sqrt(np.mean(ref ** 2))
            print(f"AZSTEP look W{width} {n_az}x{n_rg} looks {looks}: rel_l2 {err:.3e} worst cell {worst:.3e}")
            assert err <= 1e-5, (looks, err)
            assert (guard == 0xFF).all()
            e = az.step_errors(d_out.download(np.complex64, x.shape), img)          # the image itself is written as without the slot
            assert e["rel_l2"] <= az.REL_L2_MAX and e["row"] <= az.ROW_MAX, e
        if width == 16:
            d_slot = ctx.alloc(4096)
            with pytest.raises(sx.SarxError):
                plan.set_look_slot(32, d_slot.ptr)
            d_slot.release()
    finally:
        plan.set_look_slot(4, None)
        d_in.release(); d_out.release()


def _masked_phase_err(got, ref, mask):
    d = np.angle(np.exp(1j * (got[mask].astype(np.float64) - ref[mask])))
    return float(np.linalg.norm(d) / max(np.linalg.norm(ref[mask]), 1e-30))


@pytest.mark.parametrize("keep", [False, True], ids=["planes_only", "keep_image"])
@pytest.mark.parametrize("n_az,n_rg", [(1024, 128), (2048, 256)])
def test_ati_products_at_width_32(sx, ctx, plans, monkeypatch, n_az, n_rg, keep):
    """AZ_EPI_SCALE_ATI at SARX_ATI_W=32 where the default width is 64: the three planes against orc.ati_dpca of (slc1, the oracle's
    image), against the separate ATI launch on the finished image bit for bit (test_ati_products_fused_into_second_focus's bounds),
    and bit for bit equal to the width-64 planes (the same arithmetic per column)."""
    from sarx import _ffi
    plan = plans(monkeypatch, n_az, n_rg, {})
    px = n_az * n_rg
    frac, cal = 0.05, 0.3
    slc1, s3 = az.noise(n_az, n_rg, 31), az.noise(n_az, n_rg, 32)
    img = orc.azimuth_ifft_cols(s3)
    ref = orc.ati_dpca(slc1, img, mask_frac=frac, cal_phase=cal)
    d_s1, d_in, d_max = ctx.to_device(slc1), ctx.to_device(s3), ctx.alloc(_ffi.MAX_SLOT_BYTES)
    d_plain, d_img = ctx.alloc(px * 8), ctx.alloc(px * 8)
    names = ("ati_phase", "slc1_mag", "dpca_mag")
    bufs = {w: {k: ctx.alloc(px * 4) for k in names} for w in ("32", "64", "sep")}
    try:
        plan.run_pass(_ffi.PASS_AZ_IFFT, d_in, d_plain)                     # the finished second image, no epilogue
        # what the first channel's focus leaves in the max slot: the device's own hypotf of slc1 (NumPy's differs in the last bit)
        mx0, _ = ctx.ati_dpca(d_s1, d_plain, px, cal, bufs["sep"])
        assert abs(mx0 - ref["max_mag"]) <= MAX_REL * ref["max_mag"]
        shards = np.zeros((256, 32), np.float32)
        shards[0, 0] = mx0
        d_max.upload(shards)
        ctx.ati_dpca_masked(d_s1, d_plain, px, cal, d_max, frac, bufs["sep"])
        mx, sm = ctx.ati_stats()
        got, sums = {}, {}
        for w in ("64", "32"):
            monkeypatch.setenv("SARX_ATI_W", w)
            ctx.lib.sarx_memset(ctx.h, d_img.ptr, 0x5A, px * 8)
            plan.set_ati(d_s1, d_max, frac, cal, bufs[w]["ati_phase"], bufs[w]["slc1_mag"], bufs[w]["dpca_mag"], keep_image=keep)
            plan.run_pass(_ffi.PASS_AZ_IFFT, d_in, d_img)
            plan.set_ati(None)
            sums[w] = ctx.ati_stats()
            got[w] = {k: bufs[w][k].download(np.float32, (n_az, n_rg)) for k in names}
            out = d_img.download(np.uint8, (px * 8,))
            if keep:
                np.testing.assert_array_equal(out, d_plain.download(np.uint8, (px * 8,)))
            else:
                assert (out == 0x5A).all()                                  # planes only: the image is not written
        monkeypatch.delenv("SARX_ATI_W")
        sep = {k: bufs["sep"][k].download(np.float32, (n_az, n_rg)) for k in names}
        for k in names:
            np.testing.assert_array_equal(got["32"][k], sep[k])
            np.testing.assert_array_equal(got["32"][k], got["64"][k])
        for w in ("32", "64"):
            assert sums[w][0] == mx and abs(sums[w][1] - sm) <= 1e-12 * abs(sm)
        g = got["32"]
        inside = ref["slc1_mag"] > frac * ref["max_mag"] * (1 + 1e-4)       # away from the threshold: no borderline pixel
        outside = ref["slc1_mag"] < frac * ref["max_mag"] * (1 - 1e-4)
        assert 20 < inside.sum() and 20 < outside.sum()
        figs = (_masked_phase_err(g["ati_phase"], ref["ati_phase"], inside), orc.rel_l2(g["slc1_mag"], ref["slc1_mag"]),
                orc.rel_l2(g["dpca_mag"], ref["dpca_mag"]))
        print(f"AZSTEP ati W32 {n_az}x{n_rg} keep={keep}: phase {figs[0]:.3e} slc1_mag {figs[1]:.3e} dpca_mag {figs[2]:.3e}")
        assert figs[0] < 1e-4 and figs[1] < 1e-4 and figs[2] < 1e-4, figs
        assert (g["ati_phase"][outside] == 0).all() and np.count_nonzero(g["ati_phase"][inside]) > 0
    finally:
        plan.set_ati(None)
        for b in [d_s1, d_in, d_max, d_plain, d_img] + [b for d in bufs.values() for b in d.values()]:
            b.release()
