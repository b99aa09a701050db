"""The GMTI tracker on the GPU (sarx.gmti_track, sarx.GmtiTracker, TwoChannelBatch(track=...); csrc/track.hip) against the NumPy
restatement of its semantics (tests/_track_numpy.py).  The tracker works on report lists: the tests upload synthetic slots as
bytes, nothing is focused except in the batch test.

Bars: counters, ids, status, assoc and error fields equal the restatement's exactly; the fp64 states to 1e-12 relative (every
operation of the header is one IEEE operation on both sides, so in fact the bytes agree - printed, and asserted where the test is
about bytes)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _track_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu

INT_FIELDS = ("id", "status", "hits", "misses", "age", "hist", "last_frame", "last_report")
F64_FIELDS = ("p_i", "p_j", "v_i", "v_j", "sum_re", "sum_im", "sum_power", "max_ratio")


def _tp(p):
    import sarx
    return sarx.TrackParams(gate=(p["gate_az"], p["gate_rg"]), alpha=p["alpha"], beta=p["beta"], confirm=(p["confirm_hits"], p["confirm_window"]),
                            max_misses=p["max_misses"], birth_ratio=p["birth_ratio"], max_tracks=p["max_tracks"],
                            max_detections=p["max_detections"])


def _slots(frames, p):
    """frames: report arrays or (reports, count, overflow) -> the stack of slots as bytes [n_frames x slot]."""
    out = []
    for fr in frames:
        rep, count, ovf = fr if isinstance(fr, tuple) else (fr, None, 0)
        out.append(ref.slot_bytes(rep, p["max_detections"], count, ovf))
    return np.stack(out)


class _Device:
    """The low-level calls on one stack of slots: steps one by one (the table after every step) or the whole run."""

    def __init__(self, frames, p):
        import sarx
        from sarx import track
        self.ctx, self.trk, self.p = sarx.default_context(), track, p
        self.cp = _tp(p).c_params()
        self.stack = _slots(frames, p)
        self.n = len(self.stack)
        self.bufs = [self.ctx.to_device(self.stack), self.ctx.alloc(track.table_bytes(self.cp)), self.ctx.alloc(track.workspace_bytes(self.cp)),
                     self.ctx.alloc(self.n * p["max_detections"] * 4)]

    def _assoc(self):
        return self.bufs[3].download(np.int32, (self.n, self.p["max_detections"]))

    def steps(self):
        d_stack, table, ws, assoc = self.bufs
        md, stride = self.p["max_detections"], self.stack.shape[1]
        self.ctx.lib.sarx_memset(self.ctx.h, assoc.ptr, 0x55, assoc.nbytes)
        self.trk.enqueue_init(self.ctx, self.cp, table.ptr)
        tables = []
        for f in range(self.n):
            self.trk.enqueue_step(self.ctx, self.cp, d_stack.ptr + f * stride, f, table.ptr, assoc.ptr + f * md * 4, ws.ptr)
            tables.append(table.download(np.uint8, (table.nbytes,)))
        return tables, self._assoc()

    def run(self):
        d_stack, table, ws, assoc = self.bufs
        self.ctx.lib.sarx_memset(self.ctx.h, assoc.ptr, 0xAA, assoc.nbytes)
        self.ctx.lib.sarx_memset(self.ctx.h, ws.ptr, 0xAA, ws.nbytes)
        self.trk.enqueue_init(self.ctx, self.cp, table.ptr)
        self.trk.enqueue_run(self.ctx, self.cp, d_stack.ptr, self.stack.shape[1], self.n, table.ptr, assoc.ptr, ws.ptr)
        return table.download(np.uint8, (table.nbytes,)), self._assoc()

    def close(self):
        for b in self.bufs:
            b.release()


def _compare(raw, t, what):
    """A device table against the restatement's Tracker: integers exactly, fp64 states to 1e-12; returns whether the bytes agree."""
    hdr = raw[:64].view(ref.HEADER_DTYPE)[0]
    slots = raw[64:].view(ref.SLOT_DTYPE)
    for k in ref.HEADER_DTYPE.names:
        assert np.array_equal(hdr[k], t.hdr[k]), (what, k, hdr[k], t.hdr[k])
    for k in INT_FIELDS:
        np.testing.assert_array_equal(slots[k], t.slots[k], err_msg=f"{what}: {k}")
    for k in F64_FIELDS:
        np.testing.assert_allclose(slots[k], t.slots[k], rtol=1e-12, atol=0, err_msg=f"{what}: {k}")
    return np.array_equal(raw, t.table_bytes())


# ---- parity over the wave and workgroup edges -----------------------------------------------------------------------------------
COUNTS = [0, 1, 63, 64, 65, 255, 257, 1023, 1025, 1023, 257, 65, 1, 0, 0, 64, 1025, 255]
STARTS = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 200, 300, 0, 0, 0, 0, 500]      # the first mover of the pool each frame reports


def _edge_frames(seed=5):
    """A pool of 1100 movers on rows of their own (3 rows apart: neighbouring gates overlap in azimuth), frame f reporting the
    COUNTS[f] of them from STARTS[f] on at the rounded pixel: the number of live tracks follows the counts up and - two misses drop
    a track - down again, across 64, 256 and 1024.  Frame 12 reports one mover whose track was dropped the frame before while 200
    others are dropped: its birth takes slot 0, freed in that very step."""
    rng = np.random.default_rng(seed)
    k = np.arange(1100)
    j0 = rng.uniform(100, 4000, 1100)
    vj = rng.uniform(-1.5, 1.5, 1100)
    vi = rng.uniform(-0.4, 0.4, 1100)
    frames = []
    for f, c in enumerate(COUNTS):
        w = slice(STARTS[f], STARTS[f] + c)
        ij = np.stack([10 + 3 * k[w] + np.rint(vi[w] * f).astype(np.int64), np.rint(j0[w] + vj[w] * f).astype(np.int64)], axis=1)
        rep = ref.make_reports(ij, rng)
        assert len(rep) == c
        frames.append(rep)
    return frames


@pytest.fixture(scope="module")
def edge_case():
    p = ref.params(max_tracks=2048, max_detections=1536, max_misses=1)
    frames = _edge_frames()
    t = ref.Tracker(p)
    states = []
    for f, fr in enumerate(frames):
        t.step(fr, f)
        states.append((t.hdr.copy(), t.slots.copy()))
    return p, frames, t, states


def test_parity_with_the_restatement_step_by_step(edge_case):
    p, frames, t, states = edge_case
    live = [int(h["n_live"]) for h, _ in states]
    assert max(live) > 1024 and min(live[2:]) < 64 and any(64 < x < 256 for x in live) and any(256 < x < 1024 for x in live)
    drops = np.diff([int(h["drops_total"]) for h, _ in states])
    births = np.diff([int(h["births_total"]) for h, _ in states])
    assert drops[11] == 200 and births[11] == 1 and states[12][1]["id"][0] == states[12][0]["next_id"] - 1     # births, drops and slot reuse in one step
    d = _Device(frames, p)
    try:
        tables, assoc = d.steps()
    finally:
        d.close()
    same = True
    for f, raw in enumerate(tables):
        snap = ref.Tracker(p)
        snap.hdr, snap.slots = states[f]
        same &= _compare(raw, snap, f"frame {f}")
    np.testing.assert_array_equal(assoc, np.stack(t.assoc))
    print("live per frame", live, "- tables bit-identical to the restatement:", same)


def test_two_runs_and_the_loop_of_steps_are_byte_identical(edge_case):
    p, frames, t, _ = edge_case
    d = _Device(frames, p)
    try:
        tables, assoc_steps = d.steps()
        raw1, assoc1 = d.run()
        raw2, assoc2 = d.run()
    finally:
        d.close()
    assert np.array_equal(raw1, raw2) and np.array_equal(assoc1, assoc2)
    assert np.array_equal(raw1, tables[-1]) and np.array_equal(assoc1, assoc_steps)
    _compare(raw1, t, "run")


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_index():
    """Gates 4 x 4 and integer states straight after birth: every d2 is exact.  Two reports equidistant from one track, two tracks
    equidistant from one report - also with the equidistant tracks in different workgroups' share of the table."""
    p = ref.params(max_tracks=512, max_detections=8)
    far = [[1000 + 20 * k, 1000] for k in range(300)]                  # fills slots so that the tied tracks sit 300 slots apart
    cases = [[ref.make_reports([[10, 10]]), ref.make_reports([[8, 10], [12, 10]])],
             [ref.make_reports([[10, 10], [14, 10]]), ref.make_reports([[12, 10]])],
             [ref.make_reports([[10, 10], [10, 14]]), ref.make_reports([[10, 12]])]]
    pw = ref.params(max_tracks=512, max_detections=512)
    wide = [ref.make_reports([[10, 10]] + far + [[9000, 14]]), ref.make_reports([[10, 10]] + far + [[9000, 14]])]
    for frames, q in [(c, p) for c in cases] + [(wide, pw)]:
        t = ref.run(frames, q)
        d = _Device(frames, q)
        try:
            raw, assoc = d.run()
        finally:
            d.close()
        assert _compare(raw, t, "tie")                                 # integer states: the bytes agree
        np.testing.assert_array_equal(assoc, np.stack(t.assoc))
    # the expectations themselves, on the device's answer of the first two cases
    d = _Device(cases[0], p)
    raw, assoc = d.run()
    d.close()
    assert assoc[1][:2].tolist() == [0, -1] and raw[:4].view("<u4")[0] == 1
    d = _Device(cases[1], p)
    raw, assoc = d.run()
    d.close()
    slots = raw[64:].view(ref.SLOT_DTYPE)
    assert assoc[1][0] == 0 and slots["misses"][:2].tolist() == [0, 1] and slots["p_i"][:2].tolist() == [11.0, 14.0]


# ---- empty frames -----------------------------------------------------------------------------------------------------------------
def test_empty_frames_until_every_track_is_dropped():
    p = ref.params(max_tracks=256, max_detections=128, max_misses=2, birth_ratio=22.0)     # a tenth of the reports may not start a track
    frames, _ = ref.scenario(n_frames=6)
    frames = frames + [ref.make_reports([])] * 4
    t = ref.run(frames, p)
    d = _Device(frames, p)
    try:
        tables, assoc = d.steps()
    finally:
        d.close()
    _compare(tables[-1], t, "emptied")
    hdr = tables[-1][:64].view(ref.HEADER_DTYPE)[0]
    assert hdr["n_live"] == 0 and hdr["n_confirmed"] == 0 and hdr["drops_total"] == hdr["births_total"] > 0 and hdr["frames_done"] == 10
    assert tables[7][:4].view("<u4")[0] > 0 and tables[8][:4].view("<u4")[0] == 0     # max_misses empty frames are survived, the next is not
    assert not tables[-1][64:].any()                                   # a freed slot is all zeros
    assert (assoc[6:] == -1).all()


# ---- overflow -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flag", "count", "table"])
def test_overflow_is_sticky_and_raises(kind):
    import sarx
    p = ref.params(max_tracks=8, max_detections=16)
    ok = ref.make_reports([[10 * k, 10 * k] for k in range(1, 7)])
    if kind == "flag":
        bad = (ok, 6, 1)
    elif kind == "count":
        bad = (ok, 17, 0)
    else:
        bad = ref.make_reports([[10 * k, 10 * k] for k in range(1, 7)] + [[500 + 10 * k, 7] for k in range(3)])     # 3 births, 2 free slots
    frames = [ok, ok, bad, ok, ok]
    t = ref.run(frames, p)
    code = ref.TABLE_OVERFLOW if kind == "table" else ref.SLOT_OVERFLOW
    assert t.hdr["error"] == code and t.hdr["error_frame"] == 2 and t.hdr["frames_done"] == 2
    d = _Device(frames, p)
    try:
        tables, assoc = d.steps()
    finally:
        d.close()
    assert _compare(tables[-1], t, kind)
    hdr = tables[-1][:64].view(ref.HEADER_DTYPE)[0]
    assert hdr["error"] == code and hdr["error_frame"] == 2 and hdr["frames_done"] == 2
    assert np.array_equal(tables[2], tables[3]) and np.array_equal(tables[2], tables[4])        # later steps change nothing
    np.testing.assert_array_equal(assoc, np.stack(t.assoc))
    assert (assoc[3:] == -1).all()
    if kind == "table":
        assert assoc[2][:9].tolist().count(-1) == 3                    # the matched keep their ids, no birth is half made
    else:
        assert (assoc[2] == -1).all() and np.array_equal(tables[1][64:], tables[2][64:])
    with pytest.raises(sarx.TrackOverflowError) as e:
        sarx.gmti_track([s for s in _slots(frames, p)], _tp(p), frame_dt_s=0.1)
    assert e.value.frame == 2 and e.value.kind == ("table" if kind == "table" else "slot")


# ---- the Python interfaces ----------------------------------------------------------------------------------------------------------
def test_gmti_track_and_tracker_on_the_scenario():
    """gmti_track (one run) and GmtiTracker (step by step, host and device slots mixed) give the restatement's table on the
    scenario of tests/test_track.py, and the paths hold every target under one id."""
    import sarx
    p = ref.params()
    frames, truth = ref.scenario()
    t = ref.run(frames, p)
    res = sarx.gmti_track(frames, _tp(p), frame_dt_s=0.1, dr_m=2.0, v_ambiguity_mps=46.6)
    assert np.array_equal(res.raw, t.table_bytes()), "the table's bytes"
    np.testing.assert_array_equal(res.assoc, np.stack(t.assoc))
    ctx = sarx.default_context()
    tr = sarx.GmtiTracker(ctx, _tp(p), max_frames=len(frames))
    held = []
    for f, fr in enumerate(frames):
        if f % 2:
            held.append(ctx.to_device(ref.slot_bytes(fr, p["max_detections"])))
            tr.step(held[-1])
        else:
            tr.step(ref.slot_bytes(fr, p["max_detections"])[:16 + 48 * len(fr)])
    res2 = tr.result(0.1, 2.0, 46.6)
    tr.close()
    for b in held:
        b.release()
    assert np.array_equal(res2.raw, res.raw) and np.array_equal(res2.assoc, res.assoc) and res2.paths == res.paths
    sc = ref.score(t, frames, truth, p)
    for k, main in enumerate(sc["main"]):
        path = res.paths[main]
        seen = [f for f in range(len(frames)) if truth["det"][f][k] >= 0]
        assert path["frames"] == seen and path["reports"] == [int(truth["det"][f][k]) for f in seen]
    conf = res.tracks[res.tracks["confirmed"]]
    assert len(conf) == res.n_confirmed == 12
    np.testing.assert_allclose(conf["range_rate_mps"], conf["vel_j"] * 2.0 / 0.1, rtol=1e-15)
    assert np.all(np.abs(conf["v_los_unwrapped_mps"] - conf["range_rate_mps"]) <= 46.6 + 1e-9)


# ---- the batch ------------------------------------------------------------------------------------------------------------------------
def test_batch_tracks_equal_gmti_track_and_the_restatement():
    import sarx
    from sarx.batch import TwoChannelBatch
    ctx = sarx.default_context()
    n, frames = 1024, 6
    det = sarx.GmtiParams(guard=(3, 16), train=(8, 8), pfa=1e-6, max_detections=16384)
    tp = sarx.TrackParams(confirm=(2, 3), max_tracks=16384)
    b = TwoChannelBatch(ctx, n, frames, stack="detections", scene="c3", scene_scale=0.25, detect=det, track=tp)
    b.run()
    ctx.sync()
    res = b.tracks()
    stack = b.stack().copy()
    reports = [b.detections(f) for f in range(frames)]
    b.close()
    counts = [len(r) for r in reports]
    print("reports per frame", counts, "live", res.n_live, "confirmed", res.n_confirmed, "ids", len(res.paths))
    assert min(counts) > 0
    alone = sarx.gmti_track(reports, b.track_params, frame_dt_s=0.1, dr_m=res.dr_m, v_ambiguity_mps=res.v_ambiguity_mps)
    assert np.array_equal(res.raw, alone.raw) and np.array_equal(res.assoc, alone.assoc) and res.paths == alone.paths
    assert res.tracks.tobytes() == alone.tracks.tobytes()
    assert alone.v_ambiguity_mps == reports[0].v_ambiguity_mps
    p = ref.params(confirm_hits=2, confirm_window=3, max_tracks=16384, max_detections=16384)
    slots = [stack[f].view(np.uint8) for f in range(frames)]
    t = ref.run([s[16:16 + 48 * counts[f]].view(ref.REPORT_DTYPE) for f, s in enumerate(slots)], p)
    print("batch table bit-identical to the restatement:", _compare(res.raw, t, "batch"))
    np.testing.assert_array_equal(res.assoc, np.stack(t.assoc))
    assert res.n_confirmed >= 1                                        # the scene's movers persist
    # the same batch without track=: the stack is what it was
    b0 = TwoChannelBatch(ctx, n, frames, stack="detections", scene="c3", scene_scale=0.25, detect=det)
    assert b0.slot_bytes == 16 + 48 * 16384 and b0.track_params is None
    b0.run()
    ctx.sync()
    same = np.array_equal(b0.stack().view(np.uint8), stack.view(np.uint8))
    with pytest.raises(ValueError):
        b0.tracks()
    b0.close()
    assert same
