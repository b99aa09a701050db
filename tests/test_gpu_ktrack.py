"""The Kalman ground tracker on the GPU (sarx.ground_track, sarx.GroundTracker, include/sarx_ktrack.h, csrc/ktrack.hip) against
the NumPy restatement of its semantics (tests/_ktrack_numpy.py).  The tracker works on what a ground relocation read and wrote:
the tests upload synthetic slots, records and speeds as bytes; nothing is focused.

Bars: the table's BYTES and assoc equal the restatement's.  Every operation of the header is one IEEE operation on both sides, and
the first run on an MI355X gave the restatement's bytes in every case, so bytes are what is asserted.  The bound worked out before
that run stays for the one case whose inputs are not the restatement's own (the chain: the device's relocation and its restatement
may differ by 1e-6 m): RTOL(cond) = 16 cond(S) 2^-53 of each value's scale, cond(S) the largest condition number of an innovation
covariance among the case's pairs (1e3 - 1e5 here: the along-track variance against the speed's) - an error of one rounding in the
factor of S is amplified by no more than cond(S) on its way into the gain.  The seeded inputs are held clear of every decision
boundary by 1e-6 relative (tests/_ktrack_numpy.clear_of_boundaries, an assertion on the inputs that leaves no case out)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ktrack_numpy as ref  # noqa: E402
import _relocate_numpy as rref  # noqa: E402

pytestmark = pytest.mark.gpu

INT_FIELDS = ("id", "status", "hits", "misses", "age", "hist", "last_frame", "last_report")
EXACT_F64 = ("sum_re", "sum_im", "sum_power", "max_ratio")            # sums of the reports' own values: one addition each


def rtol(cond):
    return 16.0 * cond * 2.0 ** -53


def _kp(p):
    import sarx
    return sarx.KalmanTrackParams(sigma_pos=p["sigma_pos"], sigma_v=p["sigma_v"], sigma_v_tan=p["sigma_v_tan"], q=p["q"], gate_d2=p["gate_d2"],
                                  gate_m=p["gate_m"], confirm=(p["confirm_hits"], p["confirm_window"]), max_misses=p["max_misses"],
                                  birth_ratio=p["birth_ratio"], max_tracks=p["max_tracks"], max_detections=p["max_detections"])


def pack(frames, p, stride):
    """The three input stacks as bytes: slots [n x slot], records [n x md x 64], speeds [n x md x stride]; everything past a
    frame's count is 0xFF (NaN speeds and positions, status 0xFFFFFFFF), and at stride 64 the speeds lie at offset 0 of records
    that are otherwise noise (the resolver's)."""
    md, n = p["max_detections"], len(frames)
    slots = np.full((n, 16 + 48 * md), 0xFF, np.uint8)
    recs = np.full((n, md * 64), 0xFF, np.uint8)
    speeds = np.full((n, md * stride), 0xFF, np.uint8)
    for f, fr in enumerate(frames):
        k = len(fr["reports"])
        slots[f, :16].view("<u4")[:] = (fr.get("count", k), fr.get("overflow", 0), 0, 0)
        slots[f, 16:16 + 48 * k] = np.asarray(fr["reports"], ref.REPORT_DTYPE).view(np.uint8)
        recs[f, :64 * k] = np.asarray(fr["rec"], ref.RECORD_DTYPE).view(np.uint8)
        if stride == 64:
            speeds[f, :64 * k] = np.frombuffer(np.random.default_rng(f).bytes(64 * k), np.uint8)
        speeds[f].reshape(md, stride)[:k, :8] = np.asarray(fr["v_los"], np.float64).reshape(k, 1).view(np.uint8)
    return slots, recs, speeds


class _Device:
    """The low-level calls on one set of stacks: steps one by one (the table after every step) or the whole run."""

    def __init__(self, frames, p, stride=8):
        import sarx
        from sarx import ktrack
        self.ctx, self.kt, self.p, self.stride = sarx.default_context(), ktrack, p, stride
        self.cp = _kp(p).c_params()
        self.n, self.md = len(frames), p["max_detections"]
        self.host = pack(frames, p, stride)
        self.frames = [ktrack.c_frame(fr["t"], fr["P"], fr["V"], fr.get("index", f)) for f, fr in enumerate(frames)]
        self.bufs = [self.ctx.to_device(a) for a in self.host] + [self.ctx.alloc(ktrack.table_bytes(self.cp)), self.ctx.alloc(ktrack.workspace_bytes(self.cp)),
                                                                 self.ctx.alloc(max(self.n, 1) * self.md * 4)]

    def _assoc(self):
        return self.bufs[5].download(np.int32, (self.n, self.md))

    def steps(self):
        d_slots, d_rec, d_v, table, ws, assoc = self.bufs
        md = self.md
        self.ctx.lib.sarx_memset(self.ctx.h, assoc.ptr, 0x55, assoc.nbytes)
        self.ctx.lib.sarx_memset(self.ctx.h, ws.ptr, 0x55, ws.nbytes)
        self.kt.enqueue_init(self.ctx, self.cp, table.ptr)
        tables = []
        for f in range(self.n):
            self.kt.enqueue_step(self.ctx, self.cp, self.frames[f], d_slots.ptr + f * (16 + 48 * md), d_rec.ptr + f * md * 64,
                                 (d_v.ptr + f * md * self.stride, self.stride), table.ptr, assoc.ptr + f * md * 4, ws.ptr)
            tables.append(table.download(np.uint8, (table.nbytes,)))
        return tables, self._assoc()

    def run(self):
        d_slots, d_rec, d_v, table, ws, assoc = self.bufs
        md = self.md
        self.ctx.lib.sarx_memset(self.ctx.h, assoc.ptr, 0xAA, assoc.nbytes)
        self.ctx.lib.sarx_memset(self.ctx.h, ws.ptr, 0xFF, ws.nbytes)
        self.kt.enqueue_init(self.ctx, self.cp, table.ptr)
        self.kt.enqueue_run(self.ctx, self.cp, self.frames, (d_slots.ptr, 16 + 48 * md), (d_rec.ptr, md * 64), (d_v.ptr, self.stride, md * self.stride),
                            table.ptr, assoc.ptr, ws.ptr)
        return table.download(np.uint8, (table.nbytes,)), self._assoc()

    def close(self):
        for b in self.bufs:
            b.release()


def _compare(raw, hdr, slots, tol, what):
    """A device table against a restatement's header and slots: integers exactly and, with tol = None, every byte; else the fp64
    states within tol of their scale.  Returns (the worst scaled error, whether the bytes agree)."""
    got_h = raw[:64].view(ref.HEADER_DTYPE)[0]
    got = raw[64:].view(ref.SLOT_DTYPE)
    for k in ref.HEADER_DTYPE.names:
        assert np.array_equal(got_h[k], hdr[k]), (what, k, got_h[k], hdr[k])
    for k in INT_FIELDS + EXACT_F64:
        np.testing.assert_array_equal(got[k], slots[k], err_msg=f"{what}: {k}")
    live = slots["status"] != ref.FREE
    assert not got[~live].view(np.uint8).any(), what                   # a free slot is all zeros
    g, w = got[live], slots[live]
    worst = 0.0
    P = w["p"]
    diag = np.sqrt(np.stack([P[:, 0], P[:, 4], P[:, 7], P[:, 9]], axis=1))
    for k, sc in (("x", 1.0), ("y", 1.0), ("vx", 0.3), ("vy", 0.3), ("nis_last", 1.0), ("nis_sum", 1.0)):
        assert np.all(np.isfinite(g[k])), (what, k)
        worst = max(worst, float(np.max(np.abs(g[k] - w[k]) / np.maximum(np.abs(w[k]), sc), initial=0.0)))
    for (i, j), k in ref.TRI.items():
        assert np.all(np.isfinite(g["p"][:, k])), (what, "p", k)
        worst = max(worst, float(np.max(np.abs(g["p"][:, k] - P[:, k]) / (diag[:, i] * diag[:, j]), initial=0.0)))
    same = bool(np.array_equal(raw, np.concatenate([np.frombuffer(hdr.tobytes(), np.uint8), slots.view(np.uint8)])))
    if tol is None:
        assert same, (what, worst)
    else:
        assert worst <= tol, (what, worst, tol)
    return worst, same


def _restated(frames, p):
    """The restatement's run with the state after every step, held clear of every decision boundary."""
    t = ref.Tracker(p, keep_log=True)
    states = []
    for f, fr in enumerate(frames):
        t.step(fr["reports"], fr["rec"], fr["v_los"], dict(t=fr["t"], P=fr["P"], V=fr["V"], index=fr.get("index", f)), fr.get("count"), fr.get("overflow", 0))
        states.append((t.hdr.copy(), t.slots.copy()))
    return t, states, ref.clear_of_boundaries(t, p)


# ---- parity over the stage and workgroup edges ----------------------------------------------------------------------------------
# (reports per frame, max_tracks, v_los stride, max_detections or None = count + 5): the counts around the 64-lane wave and the
# 256-wide stage, count == max_detections, and tables of 1, 64, 257 and 1025 slots: the edges of the stages and of the 1024-thread
# resolve.  Seed 1 holds every case clear of the decision boundaries.
CASES = [(0, 64, 8, None), (1, 1, 64, None), (63, 64, 8, None), (64, 257, 64, None), (65, 64, 8, None), (255, 257, 64, None), (256, 1025, 8, None),
         (257, 257, 64, None), (1000, 1025, 8, None), (1000, 1, 64, None), (300, 64, 8, 300), (257, 1025, 64, 257), (1000, 257, 64, None)]


@pytest.mark.parametrize("count,max_tracks,stride,md", CASES, ids=[f"{c}x{t}-s{s}" + ("-full" if m else "") for c, t, s, m in CASES])
def test_parity_with_the_restatement(count, max_tracks, stride, md):
    """Four frames of tests/_ktrack_numpy.edge_scene: rival reports inside one gate, rival tracks for one report, every record
    status and a non-finite speed among the clutter, both birth forms, drops and reborn movers.  The table after every step is
    the restatement's, byte for byte (cond(S) up to 6.8e3: the bound 16 cond 2^-53 = 1.2e-11 was not needed)."""
    frames, p = ref.edge_scene(count, max_tracks, seed=1, max_detections=md)
    t, states, cond = _restated(frames, p)
    assert int(t.hdr["error"]) == ref.OK and int(t.hdr["frames_done"]) == len(frames)
    if count > 1 and max_tracks > 1:
        assert int(t.hdr["drops_total"]) > 0 and sum(len(g["gaps"]) for g in t.log) > 0      # drops, and rivals that had to be told apart
    d = _Device(frames, p, stride)
    try:
        tables, assoc = d.steps()
    finally:
        d.close()
    worst, same = 0.0, True
    for f, raw in enumerate(tables):
        w, s = _compare(raw, states[f][0], states[f][1], None, f"frame {f}")
        worst, same = max(worst, w), same and s
    np.testing.assert_array_equal(assoc, np.stack(t.assoc))
    print(f"{count} reports x {max_tracks} slots: cond(S) <= {cond:.3g}, tables bit-identical to the restatement: {same and worst == 0.0}")


def test_two_runs_and_the_loop_of_steps_are_byte_identical():
    frames, p = ref.edge_scene(257, 257, seed=1)
    t, states, cond = _restated(frames, p)
    d = _Device(frames, p, 64)
    try:
        tables, assoc_steps = d.steps()
        raw1, assoc1 = d.run()
        raw2, assoc2 = d.run()
    finally:
        d.close()
    assert np.array_equal(raw1, raw2) and np.array_equal(assoc1, assoc2)
    assert np.array_equal(raw1, tables[-1]) and np.array_equal(assoc1, assoc_steps)
    _compare(raw1, states[-1][0], states[-1][1], None, "run")


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def _exact(g, vel, f):
    P, V = ref.frame_geometry(f)
    g, vel = np.asarray(g, np.float64).reshape(-1, 2), np.asarray(vel, np.float64).reshape(-1, 2)
    d = g - P[:2]
    u = d / np.sqrt(np.sum(d * d, axis=1) + P[2] ** 2)[:, None]
    return dict(reports=ref.make_reports(len(g)), rec=ref.make_records(g), v_los=np.sum(vel * u, axis=1), t=ref.CIRCLE["dt"] * f, P=P, V=V)


def test_ties_go_to_the_smaller_index():
    """Two identical reports for one track, two identical tracks for one report - also 300 slots apart, in different workgroups'
    share of the table: both searches form d2 by one function on the same operands, so a tie is a tie on the device too."""
    p = ref.params(max_tracks=512, max_detections=512)
    g, vel = np.array([[100.0, 50.0]]), np.array([[5.0, -2.0]])
    far = np.stack([1500.0 + 150.0 * (np.arange(300) % 20), -3000.0 + 150.0 * (np.arange(300) // 20)], axis=1)
    cases = [[_exact(g, vel, 0), _exact(np.repeat(g + vel * 2.0, 2, axis=0), np.repeat(vel, 2, axis=0), 1)],
             [_exact(np.repeat(g, 2, axis=0), np.repeat(vel, 2, axis=0), 0), _exact(g + vel * 2.0, vel, 1)],
             [_exact(np.concatenate([g, far, g]), np.concatenate([vel, np.zeros((300, 2)), vel]), 0), _exact(g + vel * 2.0, vel, 1)]]
    want_assoc = [[0, -1], [0], [0]]
    for frames, want in zip(cases, want_assoc):
        t = ref.run(frames, p)
        d = _Device(frames, p)
        try:
            raw, assoc = d.run()
        finally:
            d.close()
        _compare(raw, t.hdr, t.slots, None, "tie")
        np.testing.assert_array_equal(assoc, np.stack(t.assoc))
        assert assoc[1][:len(want)].tolist() == want


# ---- errors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flag", "count", "record0", "table", "time"])
def test_errors_are_sticky_and_raise(kind):
    import sarx
    p = ref.params(max_tracks=8, max_detections=16)
    g = np.stack([200.0 * np.arange(6), np.zeros(6)], axis=1)
    vel = np.zeros((6, 2))
    ok = [_exact(g, vel, f) for f in range(5)]
    bad = dict(ok[2])
    if kind == "flag":
        bad["overflow"] = 1
    elif kind == "count":
        bad["count"] = 17
    elif kind == "record0":
        bad["rec"] = bad["rec"].copy()
        bad["rec"]["status"][0] = ref.REC_OVERFLOW
    elif kind == "table":
        bad = _exact(np.concatenate([g, [[0.0, 900.0], [300.0, 900.0], [600.0, 900.0]]]), np.zeros((9, 2)), 2)     # 3 births, 2 free slots
    else:
        bad["t"] = ok[1]["t"] - 1e-9
    frames = [ok[0], ok[1], bad, ok[3], ok[4]]
    t = ref.run(frames, p)
    code = dict(table=ref.TABLE_OVERFLOW, time=ref.TIME).get(kind, ref.SLOT_OVERFLOW)
    assert (int(t.hdr["error"]), int(t.hdr["error_frame"]), int(t.hdr["frames_done"])) == (code, 2, 2)
    d = _Device(frames, p)
    try:
        tables, assoc = d.steps()
        raw_run, assoc_run = d.run()
    finally:
        d.close()
    _compare(tables[-1], t.hdr, t.slots, None, kind)
    assert np.array_equal(raw_run, tables[-1]) and np.array_equal(assoc_run, assoc)
    assert np.array_equal(tables[2], tables[3]) and np.array_equal(tables[2], tables[4])        # later steps change nothing
    np.testing.assert_array_equal(assoc, np.stack(t.assoc))
    assert (assoc[3:] == -1).all()
    if kind == "table":
        assert assoc[2][:9].tolist() == [0, 1, 2, 3, 4, 5, -1, -1, -1]   # the matched keep their ids, no birth is half made
    else:
        assert (assoc[2] == -1).all() and np.array_equal(tables[1][64:], tables[2][64:])
    # the Python interface raises what the table says
    ctx = sarx.default_context()
    tr = sarx.GroundTracker(ctx, _kp(p), max_frames=5)
    try:
        for fr in frames:
            slot = rref.slot_bytes(fr["reports"], 16, fr.get("count"), fr.get("overflow", 0))
            tr.step(slot, fr["rec"], fr["v_los"], pos_ref=fr["P"], vel_ref=fr["V"], t=fr["t"])
        want = dict(table=sarx.TrackOverflowError, time=sarx.TrackTimeError).get(kind, sarx.GmtiOverflowError)
        with pytest.raises(want) as e:
            tr.result()
        if kind in ("table", "time"):
            assert e.value.frame == 2
    finally:
        tr.close()


def test_refusals_with_a_live_context():
    """What the device entry points add to the parameter check: NULL, misaligned and overlapping pointers, bad strides, bad frames."""
    import sarx
    from sarx import _ffi, ktrack
    ctx = sarx.default_context()
    p = ref.params(max_tracks=4, max_detections=8)
    cp = _kp(p).c_params()
    lib = ctx.lib
    tb, wb = ktrack.table_bytes(cp), ktrack.workspace_bytes(cp)
    buf = ctx.alloc(4096 + tb + wb + 4096)
    try:
        b = buf.ptr
        good = dict(fr=ktrack.c_frame(0.0, (5000.0, 0.0, 3000.0), (0.0, 218.0, 0.0), 0), slot=b, rec=b + 512, v=b + 1024, vs=8, table=b + 4096,
                    assoc=b + 2048, ws=b + 4096 + tb + 64)

        def refused(word, **kw):
            a = dict(good, **kw)
            fr = C.byref(a["fr"]) if a["fr"] is not None else None
            rc = lib.sarx_ktrack_step_dev(ctx.h, C.byref(cp), fr, a["slot"], a["rec"], a["v"], a["vs"], a["table"], a["assoc"], a["ws"])
            msg = lib.sarx_last_error(ctx.h).decode()
            assert rc == -1 and word in msg, (kw, rc, msg)

        for name in ("slot", "rec", "v", "table", "ws"):
            refused("NULL", **{name: None})
        refused("frame is NULL", fr=None)
        for s in (0, 4, 12, 2 ** 64 - 1):
            refused("v_los_stride", vs=s)
        for name, off in (("slot", 4), ("rec", 4), ("v", 4), ("table", 4), ("ws", 4), ("assoc", 2)):
            refused("misaligned", **{name: good[name] + off})
        refused("overlap", table=b)                                       # the table over the slot
        refused("overlap", ws=b + 512)                                    # the workspace over the records
        refused("overlap", assoc=b + 1024 + 56)                           # the assoc row over the last speed
        refused("overlap", ws=b + 4096 + tb - 8)                          # the workspace over the table's end
        refused("overlap", assoc=b + 4096)                                # the assoc row inside the table
        for k, bad in (("t", float("nan")), ("t", float("inf"))):
            fr = ktrack.c_frame(0.0, (5000.0, 0.0, 3000.0), (0.0, 218.0, 0.0), 0)
            setattr(fr, k, bad)
            refused(" t ", fr=fr)
        fr = ktrack.c_frame(0.0, (5000.0, float("nan"), 3000.0), (0.0, 218.0, 0.0), 0)
        refused("pos_ref[1]", fr=fr)
        fr = ktrack.c_frame(0.0, (5000.0, 0.0, 3000.0), (0.0, 218.0, float("inf")), 0)
        refused("vel_ref[2]", fr=fr)
        fr = ktrack.c_frame(0.0, (5000.0, 0.0, 3000.0), (0.0, 218.0, 0.0), -1)
        refused("frame_index", fr=fr)
        fr = ktrack.c_frame(0.0, (5000.0, 0.0, 3000.0), (0.0, 218.0, 0.0), 0)
        fr.reserved = 1
        refused("reserved", fr=fr)
        bad = _kp(p).c_params()
        bad.gate_m = 0.0
        rc = lib.sarx_ktrack_step_dev(ctx.h, C.byref(bad), C.byref(good["fr"]), b, b + 512, b + 1024, 8, good["table"], None, good["ws"])
        assert rc == -1 and "gate_m" in lib.sarx_last_error(ctx.h).decode()
        assert lib.sarx_ktrack_init_dev(ctx.h, C.byref(bad), good["table"]) == -1 and "gate_m" in lib.sarx_last_error(ctx.h).decode()
        assert lib.sarx_ktrack_init_dev(ctx.h, C.byref(cp), None) == -1 and "NULL" in lib.sarx_last_error(ctx.h).decode()
        assert lib.sarx_ktrack_init_dev(ctx.h, C.byref(cp), good["table"] + 4) == -1 and "misaligned" in lib.sarx_last_error(ctx.h).decode()
        # the run: its strides, its frame array, and the extents of all its frames
        two = (_ffi.KtrackFrame * 2)(good["fr"], ktrack.c_frame(2.0, (5000.0, 0.0, 3000.0), (0.0, 218.0, 0.0), 1))
        slot, recs, speeds = 16 + 48 * 8, 64 * 8, 8 * 8

        def run_refused(word, frames=two, n=2, ss=slot, rs=recs, vs=8, vf=speeds, **kw):
            a = dict(good, **kw)
            rc = lib.sarx_ktrack_run_dev(ctx.h, C.byref(cp), frames, n, a["slot"], ss, a["rec"], rs, a["v"], vs, vf, a["table"], a["assoc"], a["ws"])
            msg = lib.sarx_last_error(ctx.h).decode()
            assert rc == -1 and word in msg, (word, rc, msg)

        run_refused("n_frames", n=-1)
        run_refused("frames is NULL", frames=None)
        run_refused("slot_stride", ss=slot - 8)
        run_refused("slot_stride", ss=slot + 4)
        run_refused("records_stride", rs=recs - 64)
        run_refused("v_los_stride", vs=4)
        run_refused("v_los_frame_stride", vf=speeds - 8)
        run_refused("overlap", table=b + slot)                            # the table over the second frame's slot
        run_refused("overlap", table=b + 1024 + 2 * speeds - 8)           # the second frame's speeds reach the table
        # no frames: nothing is read, nothing is launched
        assert lib.sarx_ktrack_run_dev(ctx.h, C.byref(cp), None, 0, b, slot, b + 512, recs, b + 1024, 8, speeds, good["table"], None, good["ws"]) == 0
        # an empty slot, the optional assoc row left out
        lib.sarx_memset(ctx.h, b, 0, 4096)
        ktrack.enqueue_init(ctx, cp, good["table"])
        assert lib.sarx_ktrack_step_dev(ctx.h, C.byref(cp), C.byref(good["fr"]), b, b + 512, b + 1024, 8, good["table"], None, good["ws"]) == 0
        ctx.sync()
    finally:
        buf.release()
    assert _ffi.load().sarx_version() == 206


# ---- the chain --------------------------------------------------------------------------------------------------------------------
def test_the_chain_holds_a_steady_mover_with_its_velocity():
    """The scenario of tests/test_gpu_relocate.py's ground-tracker case - 16 frames from the 5 km circle, one mover with a steady 10
    m/s, 4 false reports per frame, two frames without the mover - with this tracker in place of the existing one:
    relocate_frames -> ground_track over the relocation's input slots, its record stack and its speeds, all left on the device.
    One confirmed track with one id and 14 hits, its velocity within 0.057 m/s of the mover's (the CPU test's figure for sigma_v =
    0.3 m/s; here the speeds are exact and the positions quantised to 2 m pixels: the restatement gives 0.024 m/s), and the table
    is the restatement's on the restatement's relocated records."""
    import sarx
    from sarx import relocate as rl
    ctx = sarx.default_context()
    c, frames, _ = rref.video_scenario()
    md, n = c["max_detections"], len(frames)
    want = rref.relocate_video(c, frames)
    p = ref.params(max_tracks=64, max_detections=md)
    kf = [dict(reports=f["reports"], rec=w[1], v_los=f["v_los"], t=c["dt"] * k, P=f["P"], V=f["V"]) for k, (f, w) in enumerate(zip(frames, want))]
    t = ref.run(kf, p, keep_log=True)
    cond = ref.clear_of_boundaries(t, p)
    d_in = ctx.to_device(np.stack([rref.slot_bytes(f["reports"], md) for f in frames]))
    v_all = np.zeros((n, md))
    for k, f in enumerate(frames):
        v_all[k, :len(f["v_los"])] = f["v_los"]
    d_v = ctx.to_device(v_all)
    stride = 16 + 48 * md

    class _At:
        def __init__(self, ptr):
            self.ptr = ptr

    slots = [_At(d_in.ptr + k * stride) for k in range(n)]
    speeds = [(d_v.ptr + k * md * 8, 8) for k in range(n)]
    geometry = [(f["P"], f["V"]) for f in frames]
    held = [d_in, d_v]
    try:
        stack, records = rl.relocate_frames(ctx, slots, speeds, geometry=geometry, grid=c["grid"], out_grid=c["out_grid"], max_detections=md)
        held += [stack, records]
        res = sarx.ground_track(slots, records, speeds, geometry=geometry, times=[c["dt"] * k for k in range(n)], params=_kp(p), ctx=ctx)
    finally:
        for x in held:
            x.release()
    # relocation on the device and its restatement may differ by 1e-6 m (the bar of tests/test_gpu_relocate.py): 1e-6 of sigma_pos in
    # an innovation, twice that in d2, a few times that after 14 updates; measured 9.5e-14
    worst, same = _compare(res.raw, t.hdr, t.slots, max(rtol(cond), 1e-5), "chain")
    np.testing.assert_array_equal(res.assoc, np.stack(t.assoc))
    conf = res.confirmed
    detections = sum(f["mover"] >= 0 for f in frames)
    ids = {int(res.assoc[k][f["mover"]]) for k, f in enumerate(frames) if f["mover"] >= 0}
    u = c["speed"] * np.array([np.cos(np.deg2rad(c["heading_deg"])), np.sin(np.deg2rad(c["heading_deg"]))])
    assert len(conf) == res.n_confirmed == 1 and int(conf["hits"][0]) == detections == 14 and ids == {int(conf["id"][0])}
    err = float(np.hypot(conf["vx"][0] - u[0], conf["vy"][0] - u[1]))
    print(f"one confirmed track, id {int(conf['id'][0])}, {int(conf['hits'][0])} hits, velocity ({conf['vx'][0]:.3f}, {conf['vy'][0]:.3f}) against "
          f"({u[0]:.3f}, {u[1]:.3f}) m/s: {err:.3f} m/s off; speed {conf['speed'][0]:.3f} m/s, heading {conf['heading'][0]:.1f} deg, "
          f"mean NIS {conf['nis_mean'][0]:.2f}; worst scaled error against the restatement {worst:.3g}")
    assert err <= 0.057
    assert abs(conf["speed"][0] - np.hypot(conf["vx"][0], conf["vy"][0])) < 1e-12 and np.allclose(conf["cov"][0], conf["cov"][0].T)
    assert abs(conf["heading"][0] - c["heading_deg"]) < 1.0
