"""The two-receiver pair and the N-receiver stack on ONE plan (csrc/tdbp_plan.h, TdbpRx): the pair runs the stack's routine on a
scratch instance of its own, so neither may see what the other left.  The stationary pair scene of tests/test_gpu_tdbp_pair.py and the
four-receiver scene of tests/test_gpu_tdbp_multi.py (160 pulses of the scaled radar both: the same plan for one grid) on 40 x 40 and on
37 x 21 with SARX_TDBP_TILE=0, and on the tile grid of those modules.  A plan has one grid, so each grid takes both scenes.  Every check
is on bytes or on an answer of the C ABI; a context of its own gives a plan no other test has touched."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_multi_numpy as ref  # noqa: E402
import _tdbp_pair_numpy as pref  # noqa: E402

pytestmark = pytest.mark.gpu
VF = (3.0, -8.0, 0.0)
HYPS = np.array([[0.0, 0.0, 0.0], [3.0, -8.0, 0.0], [9.0, 0.0, 0.0]])
RANGES_4 = ((2, 0, 9, 4), 150)       # the unaligned ranges of tests/test_gpu_tdbp_multi.py
# scene size, nx, ny, SARX_TDBP_TILE
GRIDS = {"exact-40x40": (400.0, 40, 40, "0"), "exact-37x21": (400.0, 37, 21, "0"), "tile-40x24": (10.0, 40, 24, "1")}


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@pytest.mark.parametrize("grid", list(GRIDS))
def test_pair_and_stack_on_one_plan_do_not_see_each_other(grid):
    """1 pair, stack of four, pair: the second pair's images are the first's bytes.  2 after the pair alone the stack's route query
    still refuses and its scratch reports (0, 0); after the stack's call the pair's route query reports the pair's own route.  3 a pair
    search (a 16 x 16 chip, three hypotheses, one report) before the stack's call and after it: the same records and best bytes."""
    import sarx
    from sarx import slot
    from sarx import tdbp as _tdbp
    size, nx, ny, tile = GRIDS[grid]
    route = "tile" if tile == "1" else "exact"
    two, four = pref.stationary_scene(), ref.four_rx_scene()
    assert (len(two["t_vec"]), two["num_samples"]) == (len(four["t_vec"]), four["num_samples"])   # and one waveform: one plan, held below
    rep = np.zeros(1, slot.REPORT_DTYPE)
    rep["i"], rep["j"] = ny // 2, nx // 2
    ctx = sarx.Context(0)
    try:
        def pair():
            return sarx.tdbp_pair(two["raw"][0], two["raw"][1], two["pos"], two["vel"], two["rx_offsets"], two["t_start"], two["num_samples"],
                                  two["t_vec"], size, nx, ny, vel_focus=VF, chirp_centre=two["chirp_centre"], pulse_shift=True, consts=two["k"], ctx=ctx)

        def search():
            return sarx.tdbp_pair_search(two["raw"][0], two["raw"][1], two["pos"], two["vel"], two["rx_offsets"], two["t_start"], two["num_samples"],
                                         two["t_vec"], size, nx, ny, rep, HYPS, chip=(16, 16), chirp_centre=two["chirp_centre"], pulse_shift=True,
                                         consts=two["k"], ctx=ctx)

        def answers():
            t, n, h = C.c_int(-7), C.c_uint64(), C.c_uint64()
            assert ctx.lib.sarx_tdbp_multi_scratch(plan.h, C.byref(n), C.byref(h)) == 0, ctx.last_error()
            pair_rc = ctx.lib.sarx_tdbp_pair_route(plan.h, C.byref(t))
            return pair_rc, t.value, ctx.lib.sarx_tdbp_multi_route(plan.h, C.byref(C.c_int())), (n.value, h.value)

        with _env("SARX_TDBP_TILE", tile):
            first = pair()
            plan = _tdbp.cached_plan(ctx, two["k"], len(two["t_vec"]), two["num_samples"], nx, ny)
            assert first.route == route and np.abs(first.img1).max() > 0 and np.abs(first.img2).max() > 0
            pair_rc, pair_tile, multi_rc, held = answers()
            assert (pair_rc, pair_tile) == (0, int(tile)) and multi_rc != 0 and held == (0, 0)
            found = search()
            assert found.k_best[0] >= 0 and answers() == (0, int(tile), multi_rc, (0, 0))      # the search runs on the pair's channel 1
            stack = sarx.tdbp_multi(four["raw"], four["pos"], four["vel"], four["rx_offsets"], four["t_start"], four["num_samples"], four["t_vec"],
                                    size, nx, ny, vel_focus=VF, chirp_centre=four["chirp_centre"], pulse_ranges=RANGES_4, consts=four["k"], ctx=ctx)
            assert _tdbp.cached_plan(ctx, four["k"], len(four["t_vec"]), four["num_samples"], nx, ny) is plan
            assert stack.route == route and stack.imgs.shape == (4, ny, nx) and all(np.abs(stack.imgs[c]).max() > 0 for c in range(4))
            pair_rc, pair_tile, multi_rc, held = answers()
            assert (pair_rc, pair_tile, multi_rc) == (0, int(tile), 0) and held[0] > 0
            second = pair()
            again = search()
            assert answers() == (0, int(tile), 0, held)                                         # nor do the pair's calls grow the stack's
        assert second.route == route
        assert second.img1.tobytes() == first.img1.tobytes() and second.img2.tobytes() == first.img2.tobytes()
        assert again.records.tobytes() == found.records.tobytes() and again.best.tobytes() == found.best.tobytes()
    finally:
        ctx.close()
