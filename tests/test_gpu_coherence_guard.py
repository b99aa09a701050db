"""Guard bands and poison around the two device entry points of include/sarx_coherence.h (tests/_guard.py, the protocol of
tests/test_gpu_guard.py): every device argument is a GuardedBuffer, each case runs once with every output poisoned (0xFF) and once
zeroed; the promised bytes - coh, igram, mask, the summary records - must be bit-identical and finite, optional planes that were not
asked for stay 0xFF, every zone stays clean and every input unchanged.  The workspace's content is not defined by the header: only
its extent is watched.  Results are also held against the restatement at test_gpu_coherence.py's bound."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coherence_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
BOUND = 5e-7
THR, FLOOR = 0.5, 0.5
SHAPES = [((1, 1), (16, 16)), ((65, 225), (2, 3)), ((257, 130), (16, 16))]       # 65 x 225: one row and one column past the tile
CASES = [(s, w, off, opt) for s, w in SHAPES for off in (0, 8) for opt in (True, False)]


def _id(c):
    return f"{c[0][0]}x{c[0][1]}-off{c[2]}-{'all' if c[3] else 'coh-only'}"


@pytest.mark.parametrize("shape,window,off,optional", CASES, ids=[_id(c) for c in CASES])
def test_pair_guard(shape, window, off, optional):
    import sarx
    K = importlib.import_module("sarx.coherence")
    ctx = sarx.default_context()
    n_az, n_rg = shape
    n = n_az * n_rg
    a, b = ref.pair(shape, "point", 77 + n_az)
    cp = sarx.CoherenceParams(window=window, threshold=THR, power_floor=FLOOR).c_params()
    z = zone_bytes(n_rg * 8)
    da, db = guarded(ctx, a, z, offset=off), guarded(ctx, b, z, offset=off)
    outs = {"coh": GuardedBuffer(ctx, n * 4, z, offset=off), "igram": GuardedBuffer(ctx, n * 8, z, offset=off),
            "mask": GuardedBuffer(ctx, n, z, offset=off), "summary": GuardedBuffer(ctx, 64, offset=off),
            "workspace": GuardedBuffer(ctx, K.workspace_bytes(cp, n_az, n_rg), offset=off)}
    try:
        opt = {k: (outs[k].ptr if optional else None) for k in ("igram", "mask", "summary", "workspace")}
        promised = {"workspace": None} if optional else {"workspace": 0, "igram": 0, "mask": 0, "summary": 0}
        findings, res = guarded_run(lambda: K.enqueue_pair(ctx, da.ptr, db.ptr, n_az, n_rg, cp, outs["coh"].ptr, opt["igram"], opt["mask"],
                                                           opt["summary"], opt["workspace"]),
                                    {"a": (da, a), "b": (db, b)}, outs, promised=promised, dtypes={"coh": F32, "igram": F32}, sync=ctx.sync)
        assert not findings, findings
        r = ref.coherence(a, b, window, THR, FLOOR)
        coh = res["poisoned"]["coh"].view(F32).reshape(shape)
        assert np.max(np.abs(coh.astype(np.float64) - np.minimum(np.abs(r["g"]), 1.0))) <= BOUND
        if optional:
            ig = res["poisoned"]["igram"].view(np.complex64).reshape(shape)
            assert np.max(np.abs(ig.astype(np.complex128) - r["g"])) <= BOUND
            if ref.clear_of_the_rule(r, THR, FLOOR):
                np.testing.assert_array_equal(res["poisoned"]["mask"].reshape(shape), r["mask"])
            sm = res["poisoned"]["summary"].view(K.SUMMARY_DTYPE)[0]
            assert np.isfinite(sm["sum_coh"]) and not sm["reserved"].any() and (int(sm["n_az"]), int(sm["n_rg"])) == shape
    finally:
        for g in [da, db] + list(outs.values()):
            g.release()


@pytest.mark.parametrize("shape,window,off,optional", CASES, ids=[_id(c) for c in CASES])
def test_stack_guard(shape, window, off, optional):
    import sarx
    K = importlib.import_module("sarx.coherence")
    ctx = sarx.default_context()
    n_az, n_rg = shape
    n, nf, lag = n_az * n_rg, 3, 1
    pairs = nf - lag
    frames = np.stack([ref.pair(shape, "point", 90 + f)[0] for f in range(nf)])
    cp = sarx.CoherenceParams(window=window, threshold=THR, power_floor=FLOOR).c_params()
    z = zone_bytes(n_rg * 8)
    # strides larger than a plane: the bytes between two planes are not the call's to write
    pad = 64
    d = guarded(ctx, frames, z, offset=off)
    size = {"coh": n * 4, "igram": n * 8, "mask": n}
    outs = {k: GuardedBuffer(ctx, (pairs - 1) * (v + pad) + v, z, offset=off) for k, v in size.items()}
    outs["summary"] = GuardedBuffer(ctx, 64 * pairs, offset=off)
    outs["workspace"] = GuardedBuffer(ctx, K.workspace_bytes(cp, n_az, n_rg), offset=off)

    def planes(k):
        m = np.zeros(outs[k].nbytes, bool)
        for f in range(pairs):
            m[f * (size[k] + pad):f * (size[k] + pad) + size[k]] = True
        return m

    try:
        opt = {k: (outs[k].ptr if optional else None) for k in ("igram", "mask", "summary", "workspace")}
        promised = {"coh": planes("coh")}
        promised.update({"igram": planes("igram"), "mask": planes("mask"), "workspace": None} if optional else
                        {"workspace": 0, "igram": 0, "mask": 0, "summary": 0})
        findings, res = guarded_run(lambda: K.enqueue_stack(ctx, d.ptr, nf, n * 8, lag, n_az, n_rg, cp, outs["coh"].ptr, n * 4 + pad,
                                                            opt["igram"], n * 8 + pad, opt["mask"], n + pad, opt["summary"], opt["workspace"]),
                                    {"frames": (d, frames)}, outs, promised=promised, dtypes={"coh": F32, "igram": F32}, sync=ctx.sync)
        assert not findings, findings
        for f in range(pairs):
            r = ref.coherence(frames[f], frames[f + lag], window, THR, FLOOR)
            coh = res["poisoned"]["coh"][f * (n * 4 + pad):f * (n * 4 + pad) + n * 4].view(F32).reshape(shape)
            assert np.max(np.abs(coh.astype(np.float64) - np.minimum(np.abs(r["g"]), 1.0))) <= BOUND
            if optional:
                sm = res["poisoned"]["summary"].view(K.SUMMARY_DTYPE)[f]
                assert int(sm["n_tested"]) == r["n_tested"] and not sm["reserved"].any()
    finally:
        for g in [d] + list(outs.values()):
            g.release()
