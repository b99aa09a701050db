"""Guard bands and poison around sarx_tdbp_pair_search_dev (tests/_guard.py, the protocol of tests/test_gpu_guard.py): records, best,
chips, both raw channels and the slot are GuardedBuffers; each case runs once with the outputs poisoned (0xFF) and once zeroed.
Every promised byte - the records, the best record and the chips of every counted report inside the grid, and the k_best alone of
one outside it - must be the same in both runs (so it was written, not accumulated into), every other output byte still poison
(the rows past the count, and everything but k_best of the report outside the grid), every zone clean, the raw pulses and the slot
bit-unchanged, and no NaN - which is what a read outside the raw pulses would bring in from their zones - may reach a figure.
Chips of 37 x 21 pixels on a 90 x 70 grid (partial tiles on both axes, chips shifted in at two corners), one and five hypotheses,
both kernels, a list that holds more than the slot counts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import tdbp_oracle as tb  # noqa: E402
import _tdbp_pair_numpy as pref  # noqa: E402
import _tdbp_pair_search_dev as dev  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
NX, NY = 90, 70
CHIP = (37, 21)
MD = 7
PLACES = [(0, 0), (NY - 1, NX - 1), (35, 45), (-1, 3), (33, 44)]          # the fourth lies outside the grid


@pytest.fixture(scope="module")
def scenes():
    """tile: 64 native pulses, 90 x 70 over 90 m; exact: the 160-pulse scene of the scaled radar over 360 m."""
    return {"tile": (pref.scene(64, tb.batch_constants(), [(-4.0, 3.0, 30.0), (6.0, -5.0, 12.0)], [(1.0, 2.0, 20.0, (2.0, 6.0, 0.0))]), 90.0),
            "exact": (pref.stationary_scene(), 360.0)}


@pytest.mark.parametrize("with_chips", [True, False], ids=["chips", "nochips"])
@pytest.mark.parametrize("n_hyp", [1, 5])
@pytest.mark.parametrize("route", ["tile", "exact"])
def test_pair_search_guard(route, n_hyp, with_chips, scenes):
    import sarx
    sc, scene_size = scenes[route]
    ctx = sarx.default_context()
    n_p, n_s = sc["raw"][0].shape
    hyps = np.array([[0.0, 0.0, 0.0], [3.0, -8.0, 0.0], [-6.0, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 5.0, 0.0]])[:n_hyp]
    slot = dev.slot_of(PLACES, MD)
    plan = sarx.TdbpPlan(ctx, n_p, n_s, NX, NY, sc["k"])
    d_raw = [guarded(ctx, r, zone_bytes(n_s * 8)) for r in sc["raw"]]
    d_slot = guarded(ctx, slot)
    chip_bytes = 2 * CHIP[0] * CHIP[1] * 16
    rec = GuardedBuffer(ctx, MD * n_hyp * dev.REC_BYTES)
    best = GuardedBuffer(ctx, MD * dev.BEST_BYTES)
    chips = GuardedBuffer(ctx, MD * n_hyp * chip_bytes, zone_bytes(CHIP[0] * 16))
    try:
        def call():
            return dev.call(ctx.lib, "sarx_tdbp_pair_search_dev", plan, sc, scene_size, True, hyps, d_raw[0].ptr, d_raw[1].ptr, d_slot.ptr, MD,
                            CHIP, "dpca", rec.ptr, best.ptr, chips.ptr if with_chips else None)

        want = dev.promised(PLACES, NX, NY, MD, n_hyp, CHIP)
        if not with_chips:
            want["chips"][:] = False
        # the figures that must be finite: the doubles of the records and of the best records (their int32 fields are not floats)
        findings, res = guarded_run(call, {"raw0": (d_raw[0], sc["raw"][0]), "raw1": (d_raw[1], sc["raw"][1]), "slot": (d_slot, slot)},
                                    {"rec": rec, "best": best, "chips": chips}, promised=want, dtypes={"chips": np.float64}, sync=ctx.sync)
        assert res["poisoned"]["return"] == 0 and res["zeroed"]["return"] == 0, ctx.last_error()
        assert not findings, findings
        tile = C.c_int(-1)
        assert ctx.lib.sarx_tdbp_pair_search_route(plan.h, C.byref(tile)) == 0 and tile.value == (1 if route == "tile" else 0)
        from sarx.tdbp_pair_search import BEST_DTYPE
        from sarx.tdbp_search import RECORD_DTYPE
        b = res["poisoned"]["best"].view(BEST_DTYPE)
        r = res["poisoned"]["rec"].view(RECORD_DTYPE).reshape(MD, n_hyp)
        inside = np.array([0 <= i < NY and 0 <= j < NX for i, j in PLACES])
        n = len(PLACES)
        assert list(b["k_best"][:n][~inside]) == [-1] and np.all(b["k_best"][:n][inside] >= 0)
        assert list(zip(b["x0"][:n][inside], b["y0"][:n][inside])) == [(0, 0), (NX - CHIP[0], NY - CHIP[1]), (45 - 18, 35 - 10), (44 - 18, 33 - 10)]
        for f in ("s2", "s4", "peak"):
            assert np.isfinite(r[f][:n][inside]).all() and np.all(r[f][:n][inside] > 0), f
        for f in ("s4_best", "interf_re", "interf_im", "p0", "p1"):
            assert np.isfinite(b[f][:n][inside]).all(), f
    finally:
        for g in (*d_raw, d_slot, rec, best, chips):
            g.release()
        plan.close()
