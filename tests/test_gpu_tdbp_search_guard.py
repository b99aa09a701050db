"""Guard bands and poison around sarx_tdbp_search_dev (tests/_guard.py, the protocol of tests/test_gpu_guard.py): the records, the
image stack and the raw pulses are GuardedBuffers; each case runs once with the outputs poisoned (0xFF) and once zeroed.  Every
promised byte - 32 n_hyp of the records, 16 n_hyp ny nx of the stack - must be the same in both runs (so it was written, not
accumulated into), every other output byte still poison, every zone clean, the raw pulses unchanged, and no NaN - which is what a
read outside the raw pulses would bring in from their zones - may reach a record or a pixel.  n_hyp 1 and 5, a ragged 37 x 21
image, both kernels, with the stack and without."""
import os
import sys

import numpy as np
import pytest

from oracle import tdbp_oracle as tb

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_search_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
NX, NY = 37, 21


@pytest.fixture(scope="module")
def scenes():
    return {"tile": tb.tdbp_scene(n_pulses=64, seed=7, k=tb.batch_constants(), swath=90.0, n_targets=3),
            "exact": tb.tdbp_scene(n_pulses=96, seed=9, k=tb.scaled_constants(), swath=400.0, n_targets=3)}


@pytest.mark.parametrize("with_stack", [True, False])
@pytest.mark.parametrize("n_hyp", [1, 5])
@pytest.mark.parametrize("route", ["tile", "exact"])
def test_search_guard(route, n_hyp, with_stack, scenes):
    import ctypes as C
    import sarx
    sc = scenes[route]
    k = sc["k"]
    ctx = sarx.default_context()
    raw = sc["raw"].astype(np.complex64)
    n_p, n_s = raw.shape
    hyps = np.ascontiguousarray((sc["v_tgt"][None, :] + np.array([[0.0, 0, 0], [40.0, 40, 0], [-40.0, 40, 0], [40.0, -40, 0], [-40.0, -40, 0]]))[:n_hyp])
    pos, vel, tp = (np.ascontiguousarray(sc[n], dtype=np.float64) for n in ("pos", "vel", "t_vec"))
    plan = sarx.TdbpPlan(ctx, n_p, n_s, NX, NY, k)
    d_raw = guarded(ctx, raw, zone_bytes(n_s * 8))
    rec = GuardedBuffer(ctx, 32 * n_hyp + 64)                         # 64 bytes more than promised: they must stay poison
    stack = GuardedBuffer(ctx, 16 * n_hyp * NY * NX + 64, zone_bytes(NX * 16))
    try:
        def call():
            return ctx.lib.sarx_tdbp_search_dev(plan.h, d_raw.ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(sc["t_start"]),
                                                hyps.ctypes.data, n_hyp, float(sc["swath"]), stack.ptr if with_stack else None, rec.ptr)

        findings, res = guarded_run(call, {"raw": (d_raw, raw)}, {"records": rec, "stack": stack},
                                    promised={"records": 32 * n_hyp, "stack": 16 * n_hyp * NY * NX if with_stack else 0},
                                    dtypes={"records": np.float64, "stack": np.float64}, sync=ctx.sync)
        assert res["poisoned"]["return"] == 0 and res["zeroed"]["return"] == 0, ctx.last_error()
        assert not findings, findings
        tile = C.c_int(-1)
        assert ctx.lib.sarx_tdbp_search_route(plan.h, C.byref(tile)) == 0 and tile.value == (1 if route == "tile" else 0)
        got = res["poisoned"]["records"][:32 * n_hyp].view(ref.RECORD_DTYPE)
        assert np.isfinite(got["s2"]).all() and np.isfinite(got["s4"]).all() and (got["peak"] > 0).all()
        assert ((got["peak_ix"] >= 0) & (got["peak_ix"] < NX) & (got["peak_iy"] >= 0) & (got["peak_iy"] < NY)).all()
        if with_stack:
            want = ref.records(res["poisoned"]["stack"][:16 * n_hyp * NY * NX].view(np.complex128).reshape(n_hyp, NY, NX))
            assert np.array_equal(got["peak"], want["peak"]) and np.array_equal(got["peak_ix"], want["peak_ix"])
            assert np.array_equal(got["peak_iy"], want["peak_iy"])
    finally:
        for g in (d_raw, rec, stack):
            g.release()
        plan.close()
