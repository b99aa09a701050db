"""Guard bands and poison around the device entry points of include/sarx_ktrack.h (tests/_guard.py, the protocol of
tests/test_gpu_guard.py): every device argument is a GuardedBuffer, each case runs once with every output poisoned (0xFF) and once
zeroed; the promised bytes - the whole table after init and run, the whole assoc row or block - must be bit-identical, every zone
clean and the inputs (slots, records, speeds) unchanged.  Everything past a frame's count in the reports, the records and the
speeds is 0xFF - NaN positions and speeds, a status no record has: a value read from there shows in the table or the assoc row.
The table is input and output of a step: the call uploads the state before the step afresh.  The workspace's content is not defined
by the header (scratch): only its extent is watched.  Payloads sit 0 and 8 bytes off a 16-byte boundary."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ktrack_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run  # noqa: E402
from test_gpu_ktrack import _compare, _kp, pack  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_TRACKS = 257


def _case(kind):
    """(frames, params, the restatement's header and slots before and after every step, assoc) for 0, 1 or 257 reports per frame,
    or 257 with the second frame's slot overflowed."""
    count = 257 if kind == "overflow" else int(kind)
    frames, p = ref.edge_scene(count, MAX_TRACKS, seed=1, n_frames=3)
    if kind == "overflow":
        frames[1] = dict(frames[1], overflow=1)
    t = ref.Tracker(p, keep_log=True)
    states = [(t.hdr.copy(), t.slots.copy())]
    for f, fr in enumerate(frames):
        t.step(fr["reports"], fr["rec"], fr["v_los"], dict(t=fr["t"], P=fr["P"], V=fr["V"], index=f), fr.get("count"), fr.get("overflow", 0))
        states.append((t.hdr.copy(), t.slots.copy()))
    ref.clear_of_boundaries(t, p)
    assert int(t.hdr["error"]) == (ref.SLOT_OVERFLOW if kind == "overflow" else ref.OK)
    return frames, p, states, np.stack(t.assoc)


def _bytes(state):
    return np.concatenate([np.frombuffer(state[0].tobytes(), np.uint8), state[1].view(np.uint8)])


@pytest.mark.parametrize("off", [0, 8])
def test_init_guard(off):
    import sarx
    from sarx import ktrack as K
    ctx = sarx.default_context()
    p = ref.params(max_tracks=MAX_TRACKS, max_detections=7)
    cp = _kp(p).c_params()
    table = GuardedBuffer(ctx, K.table_bytes(cp), offset=off)
    try:
        findings, res = guarded_run(lambda: K.enqueue_init(ctx, cp, table.ptr), {}, {"table": table}, sync=ctx.sync)
        assert not findings, findings
        assert np.array_equal(res["poisoned"]["table"], ref.Tracker(p).table_bytes())
    finally:
        table.release()


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("stride", [8, 64])
@pytest.mark.parametrize("kind", ["0", "1", "257", "overflow"])
def test_step_guard(kind, stride, off):
    """The second frame's step on the restatement's table after the first: matches, coasting rivals and clutter (or, overflowed,
    nothing but the error)."""
    import sarx
    from sarx import ktrack as K
    frames, p, states, assoc_ref = _case(kind)
    ctx, cp = sarx.default_context(), _kp(p).c_params()
    md, f = p["max_detections"], 1
    h_slots, h_recs, h_speeds = pack(frames, p, stride)
    slot, recs, speeds = (guarded(ctx, a[f], offset=off) for a in (h_slots, h_recs, h_speeds))
    table = GuardedBuffer(ctx, K.table_bytes(cp), offset=off)
    ws = GuardedBuffer(ctx, K.workspace_bytes(cp), offset=off)
    row = GuardedBuffer(ctx, md * 4, offset=off)
    fr = K.c_frame(frames[f]["t"], frames[f]["P"], frames[f]["V"], f)
    before = _bytes(states[f])
    try:
        def call():
            table.upload(before)
            K.enqueue_step(ctx, cp, fr, slot.ptr, recs.ptr, (speeds.ptr, stride), table.ptr, row.ptr, ws.ptr)
        findings, res = guarded_run(call, {"slot": (slot, h_slots[f]), "records": (recs, h_recs[f]), "v_los": (speeds, h_speeds[f])},
                                    {"table": table, "assoc": row, "workspace": ws}, promised={"workspace": None}, sync=ctx.sync)
        assert not findings, findings
        _compare(res["poisoned"]["table"], states[f + 1][0], states[f + 1][1], None, kind)       # the restatement's bytes
        assert np.array_equal(res["poisoned"]["assoc"].view(np.int32), assoc_ref[f])
        # without an assoc row the table is the same and the row is left alone
        row.poison()
        table.upload(before)
        K.enqueue_step(ctx, cp, fr, slot.ptr, recs.ptr, (speeds.ptr, stride), table.ptr, None, ws.ptr)
        ctx.sync()
        assert table.check_zones() == [] and row.check_zones() == [] and (row.download() == 0xFF).all()
        assert np.array_equal(table.download(), res["poisoned"]["table"])
    finally:
        for g in (slot, recs, speeds, table, ws, row):
            g.release()


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("kind", ["0", "1", "257", "overflow"])
def test_run_guard(kind, off):
    import sarx
    from sarx import ktrack as K
    frames, p, states, assoc_ref = _case(kind)
    ctx, cp = sarx.default_context(), _kp(p).c_params()
    md, n, stride = p["max_detections"], len(frames), 8
    host = pack(frames, p, stride)
    d_slots, d_recs, d_speeds = (guarded(ctx, a, offset=off) for a in host)
    table = GuardedBuffer(ctx, K.table_bytes(cp), offset=off)
    ws = GuardedBuffer(ctx, K.workspace_bytes(cp), offset=off)
    assoc = GuardedBuffer(ctx, n * md * 4, offset=off)
    cf = [K.c_frame(fr["t"], fr["P"], fr["V"], f) for f, fr in enumerate(frames)]
    try:
        def call():
            K.enqueue_init(ctx, cp, table.ptr)
            K.enqueue_run(ctx, cp, cf, (d_slots.ptr, 16 + 48 * md), (d_recs.ptr, 64 * md), (d_speeds.ptr, stride, md * stride), table.ptr, assoc.ptr,
                          ws.ptr)
        findings, res = guarded_run(call, {"slots": (d_slots, host[0]), "records": (d_recs, host[1]), "v_los": (d_speeds, host[2])},
                                    {"table": table, "assoc": assoc, "workspace": ws}, promised={"workspace": None}, sync=ctx.sync)
        assert not findings, findings
        _compare(res["poisoned"]["table"], states[-1][0], states[-1][1], None, kind)
        assert np.array_equal(res["poisoned"]["assoc"].view(np.int32).reshape(n, -1), assoc_ref)
        assoc.poison()
        K.enqueue_init(ctx, cp, table.ptr)
        K.enqueue_run(ctx, cp, cf, (d_slots.ptr, 16 + 48 * md), (d_recs.ptr, 64 * md), (d_speeds.ptr, stride, md * stride), table.ptr, None, ws.ptr)
        ctx.sync()
        assert (assoc.download() == 0xFF).all() and np.array_equal(table.download(), res["poisoned"]["table"]) and table.check_zones() == []
    finally:
        for g in (d_slots, d_recs, d_speeds, table, ws, assoc):
            g.release()
