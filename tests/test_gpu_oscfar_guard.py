"""Guard bands and poison around sarx_gmti_oscfar_dev (include/sarx_oscfar.h) with tests/_guard.py, the protocol of
tests/test_gpu_guard.py: every device argument is a GuardedBuffer, each case runs once with the slot poisoned (0xFF) and once
zeroed.  The launch is followed by sarx_gmti_refine_dev, as sarx.gmti.enqueue issues them, because only then is the order of the
list defined.  Promised are the header and the reports it counts: they must be bit-identical in both runs and equal to the
restatement; the rest of the list stays 0xFF, every zone stays clean and every input unchanged.  A list that overflowed promises
only its header.  Payloads sit 0 and 8 bytes off the allocation's alignment; the sizes are ragged against the 32 x 64 tile."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _oscfar_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

# (shape, guard, train): one tile with room to spare; one row and one column past a tile; the widest halo on a ragged plane; one row
CASES = [((5, 7), (0, 0), (1, 1)), ((33, 65), (2, 2), (8, 8)), ((97, 131), (1, 3), (31, 29)), ((1, 200), (0, 2), (0, 6))]


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("shape,guard,train", CASES, ids=[f"{c[0][0]}x{c[0][1]}" for c in CASES])
def test_oscfar_guard(shape, guard, train, off):
    import sarx
    from sarx import gmti as G
    ctx = sarx.default_context()
    n_az, n_rg = shape
    m = ref.speckle_plane(shape, 31 + n_az)
    rng = np.random.default_rng(n_rg)
    a = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    b = (a * np.exp(0.2j)).astype(np.complex64)
    rank = (3 * ref.n_full(guard, train)) // 4
    base = G.GmtiParams(guard, train, 1e-2, method="os", os_rank=rank)
    o = ref.oscfar(m, guard, train, alpha=base.resolved()[5], rank=rank)
    count = len(o["cells"])
    assert count >= 2
    z = zone_bytes(n_rg * 8)
    d_m, d_a, d_b = (guarded(ctx, x, z, offset=off) for x in (m, a, b))
    ins = {"dpca_mag": (d_m, m), "slc1": (d_a, a), "slc2": (d_b, b)}
    slots = []
    try:
        for cap in (count + 7, count, count - 1, 1):
            p = G.GmtiParams(guard, train, 1e-2, None, cap, None, "os", rank)
            slot = GuardedBuffer(ctx, p.slot_bytes(), offset=off)
            slots.append(slot)
            assert slot.nbytes == 16 + 48 * cap

            def promised(bytes_, cap=cap):
                n = int(bytes_[:4].view("<u4")[0])
                mask = np.zeros(len(bytes_), bool)
                mask[:16 + 48 * min(n, cap)] = True
                if n > cap:                                          # overflowed: which cells made it is not defined
                    mask[16:] = False
                    return {"promised": mask, "scratch": ~mask}
                return mask
            findings, res = guarded_run(lambda: G.enqueue(ctx, d_m.ptr, d_a.ptr, d_b.ptr, n_az, n_rg, p, 0.0, slot.ptr), ins, {"slot": slot},
                                        promised={"slot": promised}, sync=ctx.sync)
            assert not findings, findings
            raw = res["poisoned"]["slot"]
            n, overflow = (int(v) for v in raw[:8].view("<u4"))
            assert n == count and overflow == (1 if count > cap else 0) and not raw[8:16].any()
            if not overflow:
                rep = raw[16:16 + 48 * n].view(G.REPORT_DTYPE)
                assert list(zip(rep["i"].tolist(), rep["j"].tolist())) == o["cells"]
                assert rep["power"].tobytes() == o["power"].tobytes() and rep["mean"].tobytes() == o["level"].tobytes()
                assert np.isfinite(rep["interf_re"]).all() and np.isfinite(rep["mag1"]).all()
    finally:
        for g in [d_m, d_a, d_b] + slots:
            g.release()
