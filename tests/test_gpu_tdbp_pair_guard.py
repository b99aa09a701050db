"""Guard bands and poison around sarx_tdbp_pair_dev (tests/_guard.py, the protocol of tests/test_gpu_guard.py): both output forms
and both raw channels are GuardedBuffers; each case runs once with the outputs poisoned (0xFF) and once zeroed.  Every promised
byte - 32 ny nx of the complex128 pair, 16 ny nx of the complex64 pair - must be the same in both runs (so it was written, not
accumulated into), every other output byte still poison, every zone clean, the raw pulses unchanged, and no NaN - which is what a
read outside the raw pulses would bring in from their zones - may reach a pixel.  A ragged 37 x 21 image, both kernels, both
pulse-range settings, each output form alone and both together."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import tdbp_oracle as tb  # noqa: E402
import _tdbp_pair_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
NX, NY = 37, 21


@pytest.fixture(scope="module")
def scenes():
    """tile: 64 native pulses, 37 x 21 over 30 m; exact: the 160-pulse scene of the scaled radar over 400 m."""
    return {"tile": (ref.scene(64, tb.batch_constants(), [(-4.0, 3.0, 30.0), (6.0, -5.0, 12.0)], [(1.0, 2.0, 20.0, (2.0, 6.0, 0.0))]), 30.0),
            "exact": (ref.stationary_scene(), 400.0)}


@pytest.mark.parametrize("forms", ["both", "c128", "c64"])
@pytest.mark.parametrize("shift", [True, False], ids=["shift", "noshift"])
@pytest.mark.parametrize("route", ["tile", "exact"])
def test_pair_guard(route, shift, forms, scenes):
    import sarx
    from sarx.tdbp_pair import pair_params
    sc, scene_size = scenes[route]
    ctx = sarx.default_context()
    n_p, n_s = sc["raw"][0].shape
    pos, vel, tp = (np.ascontiguousarray(sc[n], dtype=np.float64) for n in ("pos", "vel", "t_vec"))
    vf = np.array([3.0, -8.0, 0.0])
    prm = pair_params(n_p, sc["rx_offsets"], sc["chirp_centre"], shift)
    plan = sarx.TdbpPlan(ctx, n_p, n_s, NX, NY, sc["k"])
    d_raw = [guarded(ctx, r, zone_bytes(n_s * 8)) for r in sc["raw"]]
    o128 = GuardedBuffer(ctx, 32 * NY * NX + 64, zone_bytes(NX * 16))          # 64 bytes more than promised: they must stay poison
    o64 = GuardedBuffer(ctx, 16 * NY * NX + 64, zone_bytes(NX * 8))
    try:
        def call():
            return ctx.lib.sarx_tdbp_pair_dev(plan.h, d_raw[0].ptr, d_raw[1].ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data,
                                              float(sc["t_start"]), vf.ctypes.data, scene_size, C.byref(prm), o128.ptr if forms != "c64" else None,
                                              o64.ptr if forms != "c128" else None)

        findings, res = guarded_run(call, {"raw0": (d_raw[0], sc["raw"][0]), "raw1": (d_raw[1], sc["raw"][1])}, {"c128": o128, "c64": o64},
                                    promised={"c128": 32 * NY * NX if forms != "c64" else 0, "c64": 16 * NY * NX if forms != "c128" else 0},
                                    dtypes={"c128": np.float64, "c64": np.float32}, sync=ctx.sync)
        assert res["poisoned"]["return"] == 0 and res["zeroed"]["return"] == 0, ctx.last_error()
        assert not findings, findings
        tile = C.c_int(-1)
        assert ctx.lib.sarx_tdbp_pair_route(plan.h, C.byref(tile)) == 0 and tile.value == (1 if route == "tile" else 0)
        if forms == "both":
            wide = res["poisoned"]["c128"][:32 * NY * NX].view(np.complex128)
            narrow = res["poisoned"]["c64"][:16 * NY * NX].view(np.complex64)
            assert np.abs(wide).max() > 0 and narrow.tobytes() == wide.astype(np.complex64).tobytes()
    finally:
        for g in (*d_raw, o128, o64):
            g.release()
        plan.close()
