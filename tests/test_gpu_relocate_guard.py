"""Guard bands and poison around sarx_relocate_dev (tests/_guard.py, the protocol of tests/test_gpu_guard.py): every device
argument is a GuardedBuffer; the call runs once with both outputs poisoned (0xFF) and once zeroed.  The promised bytes - 64 per
input report of the records, the header and the kept reports of the output slot - must be the same bits in both runs and finite,
everything behind them must still be 0xFF, every guard zone clean and no input written."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _relocate_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("count", [0, 1, 257, "overflow"])
def test_relocate_writes_what_it_promises_and_nothing_else(count):
    import sarx
    from sarx import relocate as rl
    ctx = sarx.default_context()
    n = 40 if count == "overflow" else count
    md = n + 23
    case = ref.seeded_case(n, 500 + n)
    if count == "overflow":
        slot = ref.slot_bytes(case["reports"], md, count=md + 5, overflow=0)
        n_rec, kept = 1, 0
        want_rec, want_hdr = ref.overflow_outputs(md + 5, md)
    else:
        slot = ref.slot_bytes(case["reports"], md)
        want_raw, want_rec, _ = ref.expected(case, md)
        n_rec, kept = n, int(want_raw[:4].view("<u4")[0])
        want_hdr = want_raw[:16]
    pad = lambda a, dt: np.concatenate([np.asarray(a, dt), np.zeros(md - n, dt)])       # noqa: E731
    host = {"slot": slot, "v_los": pad(case["v_los"], np.float64), "valid": pad(case["valid"], np.uint32),
            "v_along": pad(case["v_along"], np.float64)}
    inputs = {k: (guarded(ctx, a), a) for k, a in host.items()}
    outputs = {"records": GuardedBuffer(ctx, 64 * md), "out_slot": GuardedBuffer(ctx, 16 + 48 * md)}
    prm = rl.relocate_params(case["P"], case["V"], ref.CASE_GRID, ref.CASE_OUT, md)

    def call():
        rl.enqueue(ctx, prm, inputs["slot"][0].ptr, (inputs["v_los"][0].ptr, 8), (inputs["valid"][0].ptr, 4), (inputs["v_along"][0].ptr, 8),
                   outputs["records"].ptr, outputs["out_slot"].ptr)

    try:
        findings, res = guarded_run(call, inputs, outputs, promised={"records": 64 * n_rec, "out_slot": 16 + 48 * kept}, sync=ctx.sync)
        assert not findings, findings
        got = res["poisoned"]
        rec = got["records"][:64 * n_rec].view(ref.RECORD_DTYPE)
        for k in ("x", "y", "shift_x", "shift_y", "vx", "vy"):
            assert np.all(np.isfinite(rec[k])), k
        np.testing.assert_array_equal(rec["status"], want_rec["status"])
        np.testing.assert_array_equal(rec["rank"], want_rec["rank"])
        assert np.array_equal(got["out_slot"][:16], want_hdr)
        if count != "overflow":
            assert np.array_equal(got["out_slot"][:16 + 48 * kept], want_raw[:16 + 48 * kept])
    finally:
        for b in list(outputs.values()) + [v[0] for v in inputs.values()]:
            b.release()
    assert C.sizeof(sarx._ffi.RelocateRecord) == 64
