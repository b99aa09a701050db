"""Guard bands and poison around the device entry point of include/sarx_atigate.h (tests/_guard.py, the protocol of
tests/test_gpu_guard.py): every device argument is a GuardedBuffer, each case runs once with every output poisoned (0xFF) and once
zeroed; the promised bytes - 16 + 48 n_kept of the output slot, 96 n of the statistics - must be bit-identical in both runs and
equal to the restatement where it says so exactly, every other output byte still poison, every zone clean and the inputs (both
images, the input slot) unchanged.  Payloads sit 0 and 8 bytes off a 16-byte boundary; n = 0, 1, 1025 and the overflow, with the
statistics and without."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _atigate_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

MD = 1100                        # neither a multiple of a wave nor of the workgroup
N_AZ, N_RG = 96, 80
KW = dict(k_sigma=1.0)


@pytest.fixture(scope="module")
def scene():
    return ref.parity_scene(31, N_AZ, N_RG)


def _frame(kind, scene):
    a, b = scene
    n = {"empty": 0, "one": 1, "many": 1025, "overflow": 40}[kind]
    flat = np.random.default_rng(n + 1).choice(N_AZ * N_RG, n, replace=False)
    rep = ref.make_reports(np.stack([flat // N_RG, flat % N_RG], axis=1), seed=n)
    kw = dict(overflow=1) if kind == "overflow" else {}
    return ref.slot_bytes(rep, MD, **kw), ref.gate(rep, a, b, max_detections=MD, **KW, **kw), len(rep)


@pytest.fixture(scope="module")
def frames(scene):
    return {k: _frame(k, scene) for k in ("empty", "one", "many", "overflow")}


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("with_stats", [True, False])
@pytest.mark.parametrize("kind", ["empty", "one", "many", "overflow"])
def test_step_guard(kind, with_stats, off, frames, scene):
    import sarx
    from sarx import atigate as K
    a, b = scene
    raw, want, n = frames[kind]
    ctx = sarx.default_context()
    cp = sarx.AtiGateParams(**KW).c_params(MD)
    zone = zone_bytes(N_RG * 8)
    d_a, d_b = guarded(ctx, a, zone, offset=off), guarded(ctx, b, zone, offset=off)
    d_in = guarded(ctx, raw, offset=off)
    out = GuardedBuffer(ctx, 16 + 48 * MD, offset=off)
    stats = GuardedBuffer(ctx, 96 * MD, offset=off)
    try:
        k = want.n_kept
        n_stats = 0 if (kind == "overflow" or not with_stats) else n
        findings, res = guarded_run(
            lambda: K.enqueue_step(ctx, cp, d_a.ptr, d_b.ptr, N_AZ, N_RG, d_in.ptr, out.ptr, stats.ptr if with_stats else None),
            {"slc1": (d_a, a), "slc2": (d_b, b), "slot_in": (d_in, raw)}, {"slot_out": out, "stats": stats},
            promised={"slot_out": 16 + 48 * k, "stats": 96 * n_stats}, sync=ctx.sync)
        assert not findings, findings
        r = res["poisoned"]
        assert r["slot_out"][:16].view("<u4").tolist() == want.header.tolist()
        if want.reports is not None:
            assert np.array_equal(r["slot_out"][16:16 + 48 * k], want.reports.view(np.uint8))
            if with_stats:
                got = r["stats"][:96 * n].view(ref.STAT_DTYPE)
                for name in ("n_train", "n_look", "status", "reason", "out_index", "reserved"):
                    assert np.array_equal(got[name], want.stats[name]), name
                assert np.isfinite(r["stats"][:96 * n].view(ref.STAT_DTYPE)["psi"]).all()
    finally:
        for g in (d_a, d_b, d_in, out, stats):
            g.release()
