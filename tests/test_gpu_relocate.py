"""The ground relocation of GMTI reports on the device (sarx.ground_relocate, sarx.relocate_frames, include/sarx_relocate.h)
against its fp64 NumPy restatement (tests/_relocate_numpy.py).

Bars: status, rank, flags, the output slot's header, (i, j), order and copied bytes exactly; x, y, shift and velocity within 1e-6 m
(m/s): the device contracts products into fused multiply-adds where NumPy rounds each (relative 1e-16 on coordinates of 1e4 m is
1e-12 m, and the subtraction rho2 - al^2 amplifies it by the 1e2 the CPU round trip allows for); the seeded cases are held
clear of every decision boundary by 1e-6 (tests/_relocate_numpy.expected), so no report is left out of the exact comparisons."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _relocate_numpy as ref  # noqa: E402
import _tdbp_multi_numpy as mref  # noqa: E402
import _track_numpy as tref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
F64 = ("x", "y", "shift_x", "shift_y", "vx", "vy")


class _Run:
    """One sarx_relocate_dev on device buffers the test owns, outputs poisoned first; v_los at stride 8 from an array of its own, or
    at stride 64 out of an array of resolver records (v_los at offset 0, the valid word = their status at offset 60)."""

    def __init__(self, case, md, stride=8, out_grid=ref.CASE_OUT, grid=ref.CASE_GRID, slot=None):
        import sarx
        from sarx import relocate as rl
        from sarx.tdbp_multi import RECORD_DTYPE as multi_record
        self.ctx, self.rl, self.md, self.held = sarx.default_context(), rl, md, []
        ctx = self.ctx
        rep = case["reports"]
        n = len(rep)
        self.prm = rl.relocate_params(case["P"], case["V"], grid, out_grid, md)
        self.d_slot = self._up(ref.slot_bytes(rep, md) if slot is None else slot)
        pad = lambda a, dt: np.concatenate([np.asarray(a, dt), np.zeros(md - n, dt)])       # noqa: E731
        if stride == 8:
            self.v = (self._up(pad(case["v_los"], np.float64)).ptr, 8)
            self.valid = (None, 0) if case["valid"] is None else (self._up(pad(case["valid"], np.uint32)).ptr, 4)
        else:
            assert stride == 64 == multi_record.itemsize and multi_record.fields["status"][1] == 60 and multi_record.fields["v_los"][1] == 0
            mrec = np.frombuffer(np.random.default_rng(n).bytes(64 * md), multi_record).copy()     # every other field: noise
            mrec["v_los"][:n] = case["v_los"]
            mrec["status"][:n] = 0 if case["valid"] is None else case["valid"]
            d = self._up(mrec)
            self.v, self.valid = (d.ptr, 64), (d.ptr + 60, 64)
        self.along = (None, 0) if case["v_along"] is None else (self._up(pad(case["v_along"], np.float64)).ptr, 8)
        self.d_rec = self._hold(ctx.alloc(64 * md))
        self.d_out = self._hold(ctx.alloc(16 + 48 * md))

    def _hold(self, b):
        self.held.append(b)
        return b

    def _up(self, a):
        return self._hold(self.ctx.to_device(a))

    def go(self):
        for b in (self.d_rec, self.d_out):
            self.ctx.lib.sarx_memset(self.ctx.h, b.ptr, 0xFF, b.nbytes)
        self.rl.enqueue(self.ctx, self.prm, self.d_slot.ptr, self.v, self.valid, self.along, self.d_rec.ptr, self.d_out.ptr)
        return self.d_rec.download(np.uint8, (self.d_rec.nbytes,)), self.d_out.download(np.uint8, (self.d_out.nbytes,))

    def close(self):
        for b in self.held:
            b.release()


def _compare(rec_raw, out_raw, want_raw, want_rec, n, what):
    """The device's records and output slot against the restatement's; everything behind them still poison."""
    got = rec_raw[:64 * n].view(ref.RECORD_DTYPE)
    for k in ("status", "rank", "flags", "reserved"):
        np.testing.assert_array_equal(got[k], want_rec[k], err_msg=f"{what}: {k}")
    worst = 0.0
    for k in F64:
        assert np.all(np.isfinite(got[k])), (what, k)
        worst = max(worst, float(np.max(np.abs(got[k] - want_rec[k]), initial=0.0)))
    assert worst <= TOL, (what, worst)
    kept = int(want_raw[:4].view("<u4")[0])
    assert np.array_equal(out_raw[:16 + 48 * kept], want_raw[:16 + 48 * kept]), what       # header, (i, j), order, every copied byte
    assert np.all(rec_raw[64 * n:] == 0xFF) and np.all(out_raw[16 + 48 * kept:] == 0xFF), what
    return worst


# ---- parity over the wave and LDS-stage edges ------------------------------------------------------------------------------------
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]


@pytest.mark.parametrize("stride", [8, 64])
@pytest.mark.parametrize("given", [True, False], ids=["valid+along", "neither"])
@pytest.mark.parametrize("count", COUNTS + ["full"])
def test_parity_with_the_restatement(count, given, stride):
    """Seeded lists with the same output pixel several times and every per-report status, across one wave (64) and one LDS stage
    (256); "full": count == max_detections = 300.  d_valid and d_v_along both given and both NULL (at stride 64 the valid words
    are the resolver records' status, zero when none are given)."""
    n = 300 if count == "full" else count
    md = n if count == "full" else max(n, 1) + 37
    case = ref.seeded_case(n, 100 + n, with_valid=given, with_along=given)
    want_raw, want_rec, _ = ref.expected(case, md)
    if n >= 63:
        assert set(np.unique(want_rec["status"])) == {ref.OK, ref.NO_SPEED, ref.NO_SOLUTION, ref.OFF_GRID}
        kept = want_raw[16:16 + 48 * int(want_raw[:4].view("<u4")[0])].view(ref.REPORT_DTYPE)
        assert len(np.unique(np.stack([kept["i"], kept["j"]], 1), axis=0)) < len(kept)                                           # two reports share an output pixel
    run = _Run(case, md, stride)
    try:
        rec_raw, out_raw = run.go()
    finally:
        run.close()
    worst = _compare(rec_raw, out_raw, want_raw, want_rec, n, f"{n} reports")
    print(f"{n} reports of {md}: {int(want_raw[:4].view('<u4')[0])} kept; worst |difference| {worst:.2e}")


# ---- bits, overflow ----------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    case = ref.seeded_case(1000, 1100)
    run = _Run(case, 1024)
    try:
        a, b = run.go(), run.go()
    finally:
        run.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("how", ["flag", "count"])
def test_an_overflowed_slot_is_an_error_never_a_truncated_answer(how):
    import sarx
    md = 40
    case = ref.seeded_case(md, 140)
    count, flag = (md - 3, 1) if how == "flag" else (md + 1, 0)
    slot = ref.slot_bytes(case["reports"], md, count=count, overflow=flag)
    run = _Run(case, md, slot=slot)
    try:
        rec_raw, out_raw = run.go()
    finally:
        run.close()
    want_rec, want_hdr = ref.overflow_outputs(count, md)
    assert np.array_equal(rec_raw[:64], want_rec.view(np.uint8)) and np.all(rec_raw[64:] == 0xFF)       # record 0 alone
    assert np.array_equal(out_raw[:16], want_hdr) and np.all(out_raw[16:] == 0xFF)
    kw = dict(pos_ref=case["P"], vel_ref=case["V"], grid=ref.CASE_GRID, out_grid=ref.CASE_OUT, max_detections=md)
    with pytest.raises(sarx.GmtiOverflowError):
        sarx.ground_relocate(slot, case["v_los"], **kw)
    d = sarx.default_context().to_device(slot)
    try:
        with pytest.raises(sarx.GmtiOverflowError):
            sarx.ground_relocate(d, case["v_los"], **kw)
    finally:
        d.release()


def test_ground_relocate_from_host_arrays_and_from_a_device_slot():
    """The public wrapper: host reports and arrays against the restatement, and the same list as a device slot with device arrays."""
    import sarx
    ctx = sarx.default_context()
    n, md = 257, 300
    case = ref.seeded_case(n, 357)
    want_raw, want_rec, _ = ref.expected(case, md)
    kw = dict(pos_ref=case["P"], vel_ref=case["V"], grid=ref.CASE_GRID, out_grid=ref.CASE_OUT)
    host = sarx.ground_relocate(case["reports"], case["v_los"], valid=case["valid"], v_along=case["v_along"], **kw)
    assert len(host) == n and isinstance(host, sarx.RelocateResult)
    kept = int(want_raw[:4].view("<u4")[0])
    np.testing.assert_array_equal(host.status, want_rec["status"])
    np.testing.assert_array_equal(host.records["rank"], want_rec["rank"])
    assert np.max(np.abs(host.x - want_rec["x"])) <= TOL and np.max(np.abs(host.y - want_rec["y"])) <= TOL
    assert np.array_equal(host.slot, want_raw[:16 + 48 * kept]) and len(host.reports) == kept
    assert host.reports.tobytes() == want_raw[16:16 + 48 * kept].tobytes()
    held = [ctx.to_device(ref.slot_bytes(case["reports"], md)), ctx.to_device(case["v_los"]), ctx.to_device(case["valid"]),
            ctx.to_device(case["v_along"])]
    try:
        dev = sarx.ground_relocate(held[0], (held[1], 8), valid=(held[2].ptr, 4), v_along=(held[3], 8), max_detections=md, **kw)
        assert dev.records.tobytes() == host.records.tobytes() and np.array_equal(dev.slot, host.slot)
        with pytest.raises(ValueError, match="capacity"):
            sarx.ground_relocate(held[0], (held[1], 8), **kw)
        with pytest.raises(ValueError, match="v_los"):
            sarx.ground_relocate(case["reports"], case["v_los"][:-1], **kw)
        with pytest.raises(ValueError, match="v_along"):
            sarx.ground_relocate(case["reports"], case["v_los"], v_along=case["v_along"][:5], **kw)
    finally:
        for b in held:
            b.release()


def test_refusals_with_a_live_context():
    """What sarx_relocate_dev adds to the parameter check: NULL, misaligned and overlapping pointers, bad strides."""
    import sarx
    from sarx import _ffi, relocate as rl
    ctx = sarx.default_context()
    md = 8
    prm = rl.relocate_params((0.0, -4000.0, 3000.0), (100.0, 0.0, 0.0), ref.CASE_GRID, None, md)
    buf = ctx.alloc(8192)
    try:
        b = buf.ptr
        good = dict(slot=b, v=b + 512, vs=8, valid=b + 1024, ws=4, along=b + 1536, as_=8, rec=b + 2048, out=b + 4096)

        def refused(word, **kw):
            a = dict(good, **kw)
            rc = ctx.lib.sarx_relocate_dev(ctx.h, C.byref(prm), a["slot"], a["v"], a["vs"], a["valid"], a["ws"], a["along"], a["as_"], a["rec"], a["out"])
            msg = ctx.lib.sarx_last_error(ctx.h).decode()
            assert rc == -1 and word in msg, (kw, rc, msg)

        for name in ("slot", "v", "rec", "out"):
            refused("NULL", **{name: None})
        for s in (0, 4, 12, 2 ** 64 - 1):
            refused("v_los_stride", vs=s)
            refused("v_along_stride", as_=s)
        for s in (0, 2, 6, 2 ** 64 - 1):
            refused("valid_stride", ws=s)
        for name, off in (("slot", 4), ("v", 4), ("valid", 2), ("along", 4), ("rec", 4), ("out", 4)):
            refused("misaligned", **{name: good[name] + off})
        refused("overlap", out=b)                                         # in place
        refused("overlap", rec=b + 392)                                   # the last 8 bytes of the input slot
        refused("overlap", v=b + 2048, vs=64, valid=b + 2048 + 60, ws=64)  # the speeds inside the records
        refused("overlap", along=b + 4096 + 392)
        refused("overlap", out=b + 2048 + 504)                            # the two outputs
        bad = rl.relocate_params((0.0, -4000.0, 3000.0), (100.0, 0.0, 0.0), ref.CASE_GRID, None, md)
        bad.reserved = 1
        rc = ctx.lib.sarx_relocate_dev(ctx.h, C.byref(bad), b, b + 512, 8, None, 0, None, 0, b + 2048, b + 4096)
        assert rc == -1 and "reserved" in ctx.lib.sarx_last_error(ctx.h).decode()
        # the optional arrays left out: their strides are not looked at
        ctx.lib.sarx_memset(ctx.h, b, 0, 8192)
        assert ctx.lib.sarx_relocate_dev(ctx.h, C.byref(prm), b, b + 512, 8, None, 3, None, 5, b + 2048, b + 4096) == 0
        ctx.sync()
    finally:
        buf.release()
    assert _ffi.load().sarx_version() == 206


# ---- end to end on the device ------------------------------------------------------------------------------------------------
def test_the_chain_puts_the_mover_back_where_it_is():
    """tdbp_multi(device_output) -> gmti_detect on pair(1) -> the resolver's records left on the device -> ground_relocate reading
    them in place (v_los at offset 0, status at offset 60, stride 64), on the 320-pulse scene at GRID.  The mover's report (the
    peak of |I0 - I1|) lands within the bounds of the CPU physics test (tests/test_relocate.py; b from the restatement): per axis one
    pixel spacing, along track R / |V_xy| |v_rec - v_true| more.  The records read from the device equal those from host arrays."""
    import sarx
    from sarx import slot as sl
    from sarx.tdbp_multi import RECORD_DTYPE as multi_record, resolve_params
    ctx = sarx.default_context()
    vy = 16.0
    sc = mref.three_rx_scene(vy)
    size, nx, ny = mref.GRID
    b, _ = ref.scatterer_displacement()
    d_raw = [ctx.to_device(r) for r in sc["raw"]]
    dev = sarx.tdbp_multi(d_raw, sc["pos"], sc["vel"], sc["rx_offsets"], sc["t_start"], sc["num_samples"], sc["t_vec"], size, nx, ny,
                          chirp_centre=sc["chirp_centre"], consts=sc["k"], device_output=True)
    held = []
    try:
        xs, ys = np.linspace(-size / 2, size / 2, nx), np.linspace(-size / 2, size / 2, ny)
        lam, md = sc["wavelength"], 4096
        short = dev.pair(1)
        rep = sarx.gmti_detect(short.img1, short.img2, xs, ys, wavelength_m=lam, platform_speed_mps=sc["speed"], lag_s=short.lag_s,
                               guard=(2, 2), train=(8, 8), pfa=1e-3, max_detections=md)
        n = len(rep)
        assert n >= 1
        d_slot = ctx.to_device(sl.encode(rep, md))
        d_rec = ctx.alloc(64 * md)
        held += [d_slot, d_rec]
        prm = resolve_params(dev.lags_s, lam, 30.0, 1, md)
        rc = ctx.lib.sarx_tdbp_multi_resolve_dev(ctx.h, C.byref(prm), dev.imgs[0].ptr, ny, nx, d_slot.ptr, d_rec.ptr)
        assert rc == 0, ctx.lib.sarx_last_error(ctx.h)
        P, V = sarx.reference_geometry(sc["pos"], sc["vel"], sc["t_vec"], sc["rx_offsets"][:2])
        wide = (-2000.0, -2000.0, 4.0, 4.0, 1000, 1000)
        kw = dict(pos_ref=P, vel_ref=V, grid=mref.GRID, out_grid=wide)
        got = sarx.ground_relocate(d_slot, (d_rec, 64), valid=(d_rec.ptr + 60, 64), max_detections=md, **kw)
        mrec = d_rec.download(np.uint8, (64 * md,)).view(multi_record)[:n]
        host = sarx.ground_relocate(rep, mrec["v_los"], valid=mrec["status"], **kw)
        assert got.records.tobytes() == host.records.tobytes() and got.reports.tobytes() == host.reports.tobytes()
        d = rep.detections
        cells = list(zip(d["i"].tolist(), d["j"].tolist()))
        want, aux = ref.relocate(cells, mrec["v_los"], P, V, ref.tdbp_grid(*mref.GRID), wide, valid=mrec["status"])
        np.testing.assert_array_equal(got.status, want["status"])
        assert max(np.max(np.abs(got.records[k] - want[k])) for k in F64) <= TOL
        imgs = np.stack([z.numpy() for z in dev.imgs])
        peak = ref.mover_peak(imgs)
        assert peak in cells
        r = cells.index(peak)
        assert got.status[r] == ref.OK and mrec["status"][r] == 0
        f = ref.physics_figures(vy, peak, (got.x[r], got.y[r]), float(mrec["v_los"][r]), mref.v_los_true(sc, vy), P, V, b)
        print(f"{n} reports, {len(got.reports)} kept; " + ref.physics_line(f))
        assert f["err"][0] <= f["bound"][0] and f["err"][1] <= f["bound"][1]
        assert f["before"][0] > 0.9 * 49.5 * vy
        on_chip = sarx.ground_relocate(d_slot, (d_rec, 64), valid=(d_rec.ptr + 60, 64), max_detections=md, pos_ref=P, vel_ref=V, grid=mref.GRID)
        assert on_chip.status[r] == ref.OFF_GRID and on_chip.x[r] == got.x[r]      # the mover is off the chip it was imaged on
    finally:
        dev.release()
        for x in held + d_raw:
            x.release()


# ---- the tracker in ground coordinates -------------------------------------------------------------------------------------------
def test_the_tracker_holds_a_steady_mover_in_ground_coordinates():
    """16 frames from the 5 km circle, 5 degrees and 2 s apart; one mover with a steady 10 m/s (20 m per frame), 4 false reports per
    frame.  The tracker's grid has 8 m pixels, gate = ceil(3 v dt / out_dx) = 8 pixels (the mover's step plus two pixels of
    quantisation, times the 3 of the formula).  relocate_frames -> sarx_track_run_dev confirms exactly one track, with one id and as
    many hits as the mover has detections (14: two frames miss it).  The same TrackParams on the un-relocated slots confirm none:
    in the image's 2 m pixels the mover steps 13 to 20 pixels per frame - its own 10 and the displacement R v_los / V turning with
    the aspect angle - and every report starts a track that dies.  (A gate of 3 v dt counted in image pixels, 30, would hold that
    path too: what the ground grid buys is a gate sized by the mover's own step on pixels the tracker chooses.)  The device's table
    and assoc on the relocated stack are the bytes of tests/_track_numpy.py on the restatement's relocated slots."""
    import sarx
    from sarx import relocate as rl, track
    ctx = sarx.default_context()
    c, frames, gate = ref.video_scenario()
    md, n = c["max_detections"], len(frames)
    assert gate == 8.0 and n == 16
    want = ref.relocate_video(c, frames)
    for _, rec, aux in want:
        for k in ("fi", "fj"):
            assert np.all(np.abs(aux[k] - np.rint(aux[k])) > 1e-6)                 # no output pixel on a rounding boundary
        assert np.all(rec["status"] == ref.OK)
    p = tref.params(gate_az=gate, gate_rg=gate, max_tracks=64, max_detections=md)
    tp = sarx.TrackParams(gate=(gate, gate), alpha=p["alpha"], beta=p["beta"], confirm=(p["confirm_hits"], p["confirm_window"]),
                          max_misses=p["max_misses"], birth_ratio=p["birth_ratio"], max_tracks=p["max_tracks"], max_detections=md)
    cp = tp.c_params()
    d_in = ctx.to_device(np.stack([ref.slot_bytes(f["reports"], md) for f in frames]))
    v_all = np.zeros((n, md))
    for k, f in enumerate(frames):
        v_all[k, :len(f["v_los"])] = f["v_los"]
    d_v = ctx.to_device(v_all)
    stride = tp.slot_bytes()

    class _At:
        def __init__(self, ptr):
            self.ptr = ptr

    bufs = [d_in, d_v, ctx.alloc(track.table_bytes(cp)), ctx.alloc(track.workspace_bytes(cp)), ctx.alloc(n * md * 4)]
    try:
        stack, records = rl.relocate_frames(ctx, [_At(d_in.ptr + k * stride) for k in range(n)], [(d_v.ptr + k * md * 8, 8) for k in range(n)],
                                            geometry=[(f["P"], f["V"]) for f in frames], grid=c["grid"], out_grid=c["out_grid"],
                                            max_detections=md)
        bufs += [stack, records]
        _, _, table, ws, assoc = bufs[:5]
        track.enqueue_init(ctx, cp, table.ptr)
        track.enqueue_run(ctx, cp, stack.ptr, stride, n, table.ptr, assoc.ptr, ws.ptr)
        raw = table.download(np.uint8, (table.nbytes,))
        got_assoc = assoc.download(np.int32, (n, md))
        got_stack = stack.download(np.uint8, (n, stride))
        got_rec = records.download(np.uint8, (n * md * 64,)).view(ref.RECORD_DTYPE).reshape(n, md)
    finally:
        for x in bufs:
            x.release()
    slots = []
    for k, (w_raw, w_rec, _) in enumerate(want):
        kept = int(w_raw[:4].view("<u4")[0])
        assert np.array_equal(got_stack[k][:16 + 48 * kept], w_raw[:16 + 48 * kept]), k
        np.testing.assert_array_equal(got_rec[k][:len(w_rec)]["rank"], w_rec["rank"])
        slots.append(w_raw[16:16 + 48 * kept].view(ref.REPORT_DTYPE))
    t = tref.run(slots, p)
    assert np.array_equal(raw, t.table_bytes())                                        # bit for bit, as tests/test_gpu_track.py holds it
    assert np.array_equal(got_assoc, np.stack(t.assoc))
    slots_dev = raw[64:].view(tref.SLOT_DTYPE)
    confirmed = slots_dev[slots_dev["status"] == tref.CONFIRMED]
    detections = sum(f["mover"] >= 0 for f in frames)
    ids = {int(got_assoc[k][want[k][1]["rank"][f["mover"]]]) for k, f in enumerate(frames) if f["mover"] >= 0}
    print(f"relocated: {len(confirmed)} confirmed, hits {confirmed['hits'].tolist()}, the mover's ids {ids}, {detections} detections")
    assert len(confirmed) == 1 and int(confirmed["hits"][0]) == detections == 14 and ids == {int(confirmed["id"][0])}
    plain = tref.run([f["reports"] for f in frames], p)
    print(f"un-relocated: {int(plain.hdr['n_confirmed'])} confirmed of {int(plain.hdr['births_total'])} births")
    assert int(plain.hdr["n_confirmed"]) == 0 and not np.any(plain.slots["status"] == tref.CONFIRMED)
    never = tref.Tracker(p)                                                            # and none was confirmed on the way
    for k, f in enumerate(frames):
        never.step(f["reports"], k)
        assert int(never.hdr["n_confirmed"]) == 0, k
