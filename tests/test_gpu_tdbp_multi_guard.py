"""Guard bands and poison around sarx_tdbp_multi_dev and sarx_tdbp_multi_resolve_dev (tests/_guard.py, the protocol of
tests/test_gpu_guard.py).  Every case runs once with the outputs poisoned (0xFF) and once zeroed: every promised byte - 16 n_rx ny
nx of the complex128 stack, 8 n_rx ny nx of the complex64 stack, 64 bytes per counted report - must be the same in both runs (so
it was written, not accumulated into), every other output byte still poison, every zone clean, the inputs unchanged, and no NaN -
which is what a read outside an input would bring in from its zones - may reach a result.  The stack: a ragged 37 x 21 image, three
and four receivers, both kernels, each output form alone and both together.  The resolver: reports in the corners, on the border
and outside the image, every window size, an empty slot and an overflowing one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_multi_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
NX, NY = 37, 21
FIRST, N_USED = (2, 0, 9, 4), 150     # unaligned: every channel starts and stops at another pulse


@pytest.mark.parametrize("forms", ["both", "c128", "c64"])
@pytest.mark.parametrize("route", ["tile", "exact"])
@pytest.mark.parametrize("n_rx", [3, 4])
def test_multi_guard(n_rx, route, forms):
    """The four-receiver scene (160 pulses of the scaled radar): 37 x 21 over 8 m takes the tile kernel, over 400 m the exact one."""
    import sarx
    from sarx.tdbp_multi import multi_params
    sc = ref.four_rx_scene()
    scene_size = 8.0 if route == "tile" else 400.0
    ctx = sarx.default_context()
    n_p, n_s = sc["raw"][0].shape
    pos, vel, tp = (np.ascontiguousarray(sc[n], dtype=np.float64) for n in ("pos", "vel", "t_vec"))
    vf = np.array([3.0, -8.0, 0.0])
    prm = multi_params(n_p, sc["rx_offsets"][:n_rx], sc["chirp_centre"], (FIRST[:n_rx], N_USED))
    plan = sarx.TdbpPlan(ctx, n_p, n_s, NX, NY, sc["k"])
    d_raw = [guarded(ctx, r, zone_bytes(n_s * 8)) for r in sc["raw"][:n_rx]]
    n128, n64 = 16 * n_rx * NY * NX, 8 * n_rx * NY * NX
    o128 = GuardedBuffer(ctx, n128 + 64, zone_bytes(NX * 16))                  # 64 bytes more than promised: they must stay poison
    o64 = GuardedBuffer(ctx, n64 + 64, zone_bytes(NX * 8))
    ptrs = (C.c_void_p * n_rx)(*(b.ptr for b in d_raw))                        # n_rx entries and no more
    try:
        def call():
            return ctx.lib.sarx_tdbp_multi_dev(plan.h, ptrs, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(sc["t_start"]),
                                               vf.ctypes.data, scene_size, C.byref(prm), o128.ptr if forms != "c64" else None,
                                               o64.ptr if forms != "c128" else None)

        findings, res = guarded_run(call, {f"raw{c}": (d_raw[c], sc["raw"][c]) for c in range(n_rx)}, {"c128": o128, "c64": o64},
                                    promised={"c128": n128 if forms != "c64" else 0, "c64": n64 if forms != "c128" else 0},
                                    dtypes={"c128": np.float64, "c64": np.float32}, sync=ctx.sync)
        assert res["poisoned"]["return"] == 0 and res["zeroed"]["return"] == 0, ctx.last_error()
        assert not findings, findings
        tile = C.c_int(-1)
        assert ctx.lib.sarx_tdbp_multi_route(plan.h, C.byref(tile)) == 0 and tile.value == (1 if route == "tile" else 0)
        if forms == "both":
            wide = res["poisoned"]["c128"][:n128].view(np.complex128).reshape(n_rx, NY, NX)
            narrow = res["poisoned"]["c64"][:n64].view(np.complex64)
            assert all(np.abs(wide[c]).max() > 0 for c in range(n_rx)) and narrow.tobytes() == wide.astype(np.complex64).tobytes()
    finally:
        for g in (*d_raw, o128, o64):
            g.release()
        plan.close()


def _slot(md, cells, count=None, overflow=0):
    from sarx import slot
    raw = np.zeros(slot.slot_bytes(md), np.uint8)
    rep = raw[slot.HEADER_BYTES:].view(slot.REPORT_DTYPE)
    for r, (i, j) in enumerate(cells):
        rep["i"][r], rep["j"][r] = i, j
    raw[:8].view("<u4")[:] = (len(cells) if count is None else count, overflow)
    return raw


CELLS = [(0, 0), (0, NX - 1), (NY - 1, 0), (NY - 1, NX - 1), (10, 18), (3, NX - 2), (NY + 4, 5), (5, -5), (-7, 400), (2 ** 31 - 1, -2 ** 31)]


@pytest.mark.parametrize("case", ["reports", "empty", "flag", "count"])
@pytest.mark.parametrize("half", [0, 1, 4])
@pytest.mark.parametrize("n_rx", [2, 4])
def test_resolve_guard(n_rx, half, case):
    """md = 16 slots.  reports: ten of them, the last four so far outside the image that their box misses it (status 2, nothing read); empty: count 0, nothing
    written; flag / count: the overflow flag set, or count = md + 1: record 0 alone, status 3.  The records are held to the restated
    resolver, too."""
    import sarx
    from sarx.tdbp_multi import RECORD_DTYPE, resolve_params
    ctx = sarx.default_context()
    md = 16
    rng = np.random.default_rng(7)
    imgs = (rng.standard_normal((n_rx, NY, NX)) + 1j * rng.standard_normal((n_rx, NY, NX))).astype(np.complex64)
    lags = (2e-4, -1e-3, 7.3e-4)[:n_rx - 1]
    lam, v_max = 0.03, 40.0
    prm = resolve_params(lags, lam, v_max, half, md)
    raw = {"reports": _slot(md, CELLS), "empty": _slot(md, []), "flag": _slot(md, CELLS, overflow=1), "count": _slot(md, CELLS, count=md + 1)}[case]
    want = {"reports": 64 * len(CELLS), "empty": 0, "flag": 64, "count": 64}[case]
    d_img = guarded(ctx, imgs, zone_bytes(NX * 8))
    d_slot = guarded(ctx, raw)
    d_rec = GuardedBuffer(ctx, 64 * md + 64)
    try:
        def call():
            return ctx.lib.sarx_tdbp_multi_resolve_dev(ctx.h, C.byref(prm), d_img.ptr, NY, NX, d_slot.ptr, d_rec.ptr)

        findings, res = guarded_run(call, {"images": (d_img, imgs), "slot": (d_slot, raw)}, {"records": d_rec}, promised={"records": want},
                                    sync=ctx.sync)
        assert res["poisoned"]["return"] == 0 and res["zeroed"]["return"] == 0, ctx.last_error()
        assert not findings, findings
        rec = res["poisoned"]["records"][:want].view(RECORD_DTYPE)
        if case == "reports":
            ok = rec["status"] != 2
            assert list(rec["status"][6:]) == [2] * 4 and ok[:6].all()
            for f in ("v_los", "v_coarse", "phase"):
                assert np.isfinite(rec[f]).all(), f
            ref_rec = ref.resolve(imgs, CELLS, lags, lam, v_max, half)
            np.testing.assert_array_equal(rec["status"], ref_rec["status"])
            np.testing.assert_array_equal(rec["k"], ref_rec["k"])
            assert np.max(np.abs(rec["phase"] - ref_rec["phase"])) <= 1e-12 and np.max(np.abs(rec["v_los"] - ref_rec["v_los"])) <= 1e-9
        elif case != "empty":
            assert rec["status"][0] == 3 and rec["k"][0] == 0
            assert all(rec[f][0] == 0.0 for f in ("v_los", "v_coarse", "cost", "cost_next")) and not rec["phase"][0].any()
    finally:
        for g in (d_img, d_slot, d_rec):
            g.release()
