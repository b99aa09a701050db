"""Guard bands and poison around the three device entry points of include/sarx_track.h (tests/_guard.py, the protocol of
tests/test_gpu_guard.py): every device argument is a GuardedBuffer, each case runs once with every output poisoned (0xFF) and once
zeroed; the promised bytes - the whole table after init and run, the whole assoc row or block - must be bit-identical, every zone
clean and the slots unchanged.  The table is input and output of a step: the call uploads the state before the step afresh, so
what is checked on it is the zones, the two runs' agreement and the restatement.  The workspace's content is not defined by the
header (scratch): only its extent is watched.  Payloads sit 0 and 8 bytes off a 16-byte boundary."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _track_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run  # noqa: E402

pytestmark = pytest.mark.gpu

P = ref.params(max_tracks=300, max_detections=200, max_misses=1)       # neither a multiple of a wave nor of a workgroup


@pytest.fixture(scope="module")
def case():
    frames, _ = ref.scenario(n_frames=8, n_targets=40, n_false=30)
    t = ref.Tracker(P)
    tables = [t.table_bytes().copy()]
    for f, fr in enumerate(frames):
        t.step(fr, f)
        tables.append(t.table_bytes().copy())
    assert t.hdr["drops_total"] > 0 and t.hdr["n_confirmed"] > 0
    stack = np.stack([ref.slot_bytes(fr, P["max_detections"]) for fr in frames])
    return frames, tables, np.stack(t.assoc), stack


def _cp():
    import sarx
    return sarx.TrackParams(max_tracks=P["max_tracks"], max_detections=P["max_detections"], max_misses=P["max_misses"]).c_params()


@pytest.mark.parametrize("off", [0, 8])
def test_init_guard(off, case):
    import sarx
    from sarx import track as T
    ctx, cp = sarx.default_context(), _cp()
    table = GuardedBuffer(ctx, T.table_bytes(cp), offset=off)
    try:
        findings, res = guarded_run(lambda: T.enqueue_init(ctx, cp, table.ptr), {}, {"table": table}, sync=ctx.sync)
        assert not findings, findings
        assert np.array_equal(res["poisoned"]["table"], case[1][0])
    finally:
        table.release()


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("frame", [0, 5])
def test_step_guard(off, frame, case):
    import sarx
    from sarx import track as T
    frames, tables, assoc_ref, stack = case
    ctx, cp = sarx.default_context(), _cp()
    slot = guarded(ctx, stack[frame], offset=off)
    table = GuardedBuffer(ctx, T.table_bytes(cp), offset=off)
    ws = GuardedBuffer(ctx, T.workspace_bytes(cp), offset=off)
    row = GuardedBuffer(ctx, P["max_detections"] * 4, offset=off)
    try:
        def call():
            table.upload(tables[frame])
            T.enqueue_step(ctx, cp, slot.ptr, frame, table.ptr, row.ptr, ws.ptr)
        findings, res = guarded_run(call, {"slot": (slot, stack[frame])}, {"table": table, "assoc": row, "workspace": ws},
                                    promised={"workspace": None}, sync=ctx.sync)
        assert not findings, findings
        assert np.array_equal(res["poisoned"]["table"], tables[frame + 1])
        assert np.array_equal(res["poisoned"]["assoc"].view(np.int32), assoc_ref[frame])
        # without an assoc row the table is the same and the row is left alone
        row.poison()
        table.upload(tables[frame])
        T.enqueue_step(ctx, cp, slot.ptr, frame, table.ptr, None, ws.ptr)
        ctx.sync()
        assert table.check_zones() == [] and row.check_zones() == [] and (row.download() == 0xFF).all()
        assert np.array_equal(table.download(), tables[frame + 1])
    finally:
        for g in (slot, table, ws, row):
            g.release()


@pytest.mark.parametrize("off", [0, 8])
def test_run_guard(off, case):
    import sarx
    from sarx import track as T
    frames, tables, assoc_ref, stack = case
    ctx, cp = sarx.default_context(), _cp()
    n = len(frames)
    d_stack = guarded(ctx, stack, offset=off)
    table = GuardedBuffer(ctx, T.table_bytes(cp), offset=off)
    ws = GuardedBuffer(ctx, T.workspace_bytes(cp), offset=off)
    assoc = GuardedBuffer(ctx, n * P["max_detections"] * 4, offset=off)
    try:
        def call():
            T.enqueue_init(ctx, cp, table.ptr)
            T.enqueue_run(ctx, cp, d_stack.ptr, stack.shape[1], n, table.ptr, assoc.ptr, ws.ptr)
        findings, res = guarded_run(call, {"stack": (d_stack, stack)}, {"table": table, "assoc": assoc, "workspace": ws},
                                    promised={"workspace": None}, sync=ctx.sync)
        assert not findings, findings
        assert np.array_equal(res["poisoned"]["table"], tables[-1])
        assert np.array_equal(res["poisoned"]["assoc"].view(np.int32).reshape(n, -1), assoc_ref)
        assoc.poison()
        T.enqueue_init(ctx, cp, table.ptr)
        T.enqueue_run(ctx, cp, d_stack.ptr, stack.shape[1], n, table.ptr, None, ws.ptr)
        ctx.sync()
        assert (assoc.download() == 0xFF).all() and np.array_equal(table.download(), tables[-1]) and table.check_zones() == []
    finally:
        for g in (d_stack, table, ws, assoc):
            g.release()
