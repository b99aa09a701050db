"""The GMTI plot extraction on the device (include/sarx_cluster.h, csrc/cluster.hip, sarx/cluster.py) against the flood-fill
restatement of tests/_cluster_numpy.py: synthetic slots go up as bytes, header, plot list, plot records and labels come back and
are compared - integers and labels exactly, fp64 fields to 1e-12 relative (whether they are bit-identical is printed) - then counts
known by construction, overflow, repeatability, the Python interfaces and the batch."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cluster_numpy as ref  # noqa: E402
from test_cluster import check_hand_example, hand_example  # noqa: E402

pytestmark = pytest.mark.gpu


class Out:
    """One frame's outputs as downloaded, whole buffers (poisoned with 0xFF before the launch), in the restatement's form."""

    def __init__(self, slot, plots, labels):
        self.slot, self.plots_raw, self.labels = slot, plots, labels
        self.header = slot[:16].view("<u4")
        k = min(int(self.header[0]), (len(slot) - 16) // 48)
        self.n_plots = k
        self.reports = slot[16:16 + 48 * k].view(ref.REPORT_DTYPE)
        self.plots = None if plots is None else plots[:64 * k].view(ref.PLOT_DTYPE)


def device_step(raw, link, min_members, md, want_plots=True, want_labels=True):
    """sarx_cluster_step_dev on the slot bytes `raw`."""
    import sarx
    from sarx import cluster as K
    ctx = sarx.default_context()
    cp = sarx.ClusterParams(link=link, min_members=min_members).c_params(md)
    bufs = [ctx.to_device(raw), ctx.alloc(16 + 48 * md), ctx.alloc(64 * md), ctx.alloc(4 * md)]
    try:
        d_in, d_out, d_plots, d_labels = bufs
        for b in bufs[1:]:
            sarx._ffi.check(ctx.lib.sarx_memset(ctx.h, b.ptr, 0xFF, b.nbytes), ctx.h)
        K.enqueue_step(ctx, cp, d_in.ptr, d_out.ptr, d_plots.ptr if want_plots else None, d_labels.ptr if want_labels else None)
        return Out(d_out.download(np.uint8, (d_out.nbytes,)).copy(), d_plots.download(np.uint8, (d_plots.nbytes,)).copy(),
                   d_labels.download(np.int32, (md,)).copy())
    finally:
        for b in bufs:
            b.release()


def check_case(rep, link, min_members, md, name):
    want = ref.cluster(rep, link[0], link[1], min_members, max_detections=md)
    got = device_step(ref.slot_bytes(rep, md), link, min_members, md)
    same = ref.compare(want, got.slot[:16], got.slot[16:], got.plots_raw, got.labels)
    print(f"{name}: n = {len(rep)}, plots = {want.n_plots}, fp64 fields bit-identical: {same}")
    # nothing past the plots is touched
    assert (got.slot[16 + 48 * want.n_plots:] == 0xFF).all() and (got.plots_raw[64 * want.n_plots:] == 0xFF).all()
    return want, got


def random_cells(n, seed, side=512):
    flat = np.random.default_rng(seed).choice(side * side, n, replace=False)
    return np.stack([flat // side, flat % side], axis=1)


# ---- parity with the restatement ----------------------------------------------------------------------------------------------------
# capacities: up to 4096 the kernel keeps the keys in LDS, above that it reads them from the slot; 4096 and 16384 fill the sort exactly
@pytest.mark.parametrize("n,md", [(0, 100), (1, 100), (2, 100), (63, 100), (64, 100), (65, 100), (1023, 1100), (1024, 1100), (1025, 1100),
                                  (1025, 16384), (4096, 4096), (16384, 16384)])
def test_random_cells_equal_the_restatement(n, md):
    want, got = check_case(ref.make_reports(random_cells(n, 100 + n), seed=n), (3, 5), 1, md, "random")
    assert want.n_plots <= n and (n < 1023 or want.n_plots < n)


def test_hand_example_on_the_device():
    rep = hand_example()
    for mm in (1, 2):
        got = device_step(ref.slot_bytes(rep, 12), (2, 3), mm, 12)
        check_hand_example(got, mm)


@functools.lru_cache(maxsize=None)
def shape(kind):
    if kind == "row":           # (b) one row, a report every link_rg columns, 2000 long: the label crosses 1999 links
        return ref.make_reports([[7, 5 * k] for k in range(2000)], seed=1), (3, 5), 2048
    if kind == "u":             # (c) two columns of 300 joined only along the last row: down, across and up again
        cells = [[i, j] for i in range(300) for j in (0, 40)] + [[299, j] for j in range(4, 40, 4)]
        return ref.make_reports(cells, seed=2), (1, 4), 1024
    if kind == "stairs":        # (d) j falls as i rises
        return ref.make_reports([[i, 2000 - 3 * i] for i in range(500)], seed=3), (1, 3), 600
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["row", "u", "stairs"])
def test_long_ways_give_one_plot(kind):
    rep, link, md = shape(kind)
    want, got = check_case(rep, link, 1, md, kind)
    assert got.n_plots == 1 and got.plots["n_members"][0] == len(rep) and (got.labels[:len(rep)] == 0).all()
    if kind == "stairs":        # one column less of reach and every step stands alone
        want, got = check_case(rep, (1, 2), 1, md, "stairs apart")
        assert got.n_plots == len(rep)


def test_dense_block_and_identity():
    """(e) every cell of a 64 x 64 block: one plot of 4096 members, summed by one thread; with link (0, 0) the plot list IS the
    report list, byte for byte."""
    rep = ref.make_reports([[100 + i, 200 + j] for i in range(64) for j in range(64)], seed=5)
    want, got = check_case(rep, (2, 2), 1, 4096, "dense")
    assert got.n_plots == 1 and got.plots["n_members"][0] == 4096
    assert (got.plots["i_min"][0], got.plots["i_max"][0], got.plots["j_min"][0], got.plots["j_max"][0]) == (100, 163, 200, 263)
    raw = ref.slot_bytes(rep, 4096)
    ident = device_step(raw, (0, 0), 1, 4096)
    assert np.array_equal(ident.slot, raw), "identity"
    assert np.array_equal(ident.labels, np.arange(4096)) and (ident.plots["n_members"] == 1).all()
    assert np.array_equal(ident.plots["peak_report"], np.arange(4096))


def test_equal_powers_and_minimum_size():
    # (f) a block of equal powers: the peak is the smallest index
    rep = ref.make_reports([[10 + i, 10 + j] for i in range(8) for j in range(8)], power=np.full(64, 7.0))
    want, got = check_case(rep, (1, 1), 1, 64, "equal powers")
    assert got.n_plots == 1 and got.plots["peak_report"][0] == 0 and (got.reports["i"][0], got.reports["j"][0]) == (10, 10)
    # (g) runs of 1 .. 5 adjacent cells, four of each, min_members = 3: the twelve of size 3, 4, 5 stay
    cells = [[20 * k, 30 * s + c] for k in range(4) for s in range(1, 6) for c in range(s)]
    rep = ref.make_reports(cells, seed=6)
    want, got = check_case(rep, (0, 1), 3, 100, "sizes 1 .. 5")
    assert got.n_plots == 12 and sorted(got.plots["n_members"].tolist()) == [3] * 4 + [4] * 4 + [5] * 4
    assert (got.labels[:len(rep)] == -1).sum() == 4 * (1 + 2)


def test_anisotropy():
    """(h) the same list with the link box lying and standing."""
    rep = ref.make_reports(random_cells(1500, 9, side=128), seed=9)
    a, _ = check_case(rep, (0, 7), 1, 1500, "link (0, 7)")
    b, _ = check_case(rep, (7, 0), 1, 1500, "link (7, 0)")
    assert (a.plots["i_min"] == a.plots["i_max"]).all() and (b.plots["j_min"] == b.plots["j_max"]).all()
    assert not np.array_equal(a.labels, b.labels)


# ---- known truth ------------------------------------------------------------------------------------------------------------------------
def test_twenty_seven_objects():
    """27 objects, each a 3 x 3 lattice of reports at spacing (4, 6), centres 60 cells apart: link (4, 6) reaches exactly the
    lattice neighbours - 27 plots of 9; link (3, 5) reaches nobody - 243 singletons."""
    centres = [[50 + 60 * a, 50 + 60 * b] for a in range(6) for b in range(5)][:27]
    cells = [[ci + 4 * di, cj + 6 * dj] for ci, cj in centres for di in (-1, 0, 1) for dj in (-1, 0, 1)]
    rep = ref.make_reports(cells, seed=27)
    want, got = check_case(rep, (4, 6), 1, 256, "27 objects")
    assert got.n_plots == 27 and (got.plots["n_members"] == 9).all()
    assert (got.plots["i_max"] - got.plots["i_min"] == 8).all() and (got.plots["j_max"] - got.plots["j_min"] == 12).all()
    want, got = check_case(rep, (3, 5), 1, 256, "27 objects apart")
    assert got.n_plots == 243 and (got.plots["n_members"] == 1).all()


# ---- overflow ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(overflow=1), dict(count=65)])
def test_overflow_in_overflow_out(kw):
    import sarx
    rep = ref.make_reports(random_cells(64, 11), seed=11)
    raw = ref.slot_bytes(rep, 64, **kw)
    got = device_step(raw, (3, 5), 1, 64)
    assert got.header.tolist() == [kw.get("count", 64), 1, 0, 0]
    assert (got.labels == -1).all() and (got.slot[16:] == 0xFF).all() and (got.plots_raw == 0xFF).all()
    ref.compare(ref.cluster(rep, 3, 5, 1, max_detections=64, **kw), got.slot[:16], None, None, got.labels)
    with pytest.raises(sarx.GmtiOverflowError) as e:
        sarx.gmti_cluster(raw, sarx.ClusterParams(link=(3, 5)), max_detections=64)
    assert e.value.count == kw.get("count", 64)
    with pytest.raises(sarx.GmtiOverflowError):
        sarx.gmti_cluster([raw, raw], sarx.ClusterParams(link=(3, 5)), max_detections=64)


# ---- repeatability, and the stack in one launch --------------------------------------------------------------------------------------------
def test_runs_repeat_and_the_stack_equals_the_steps():
    import sarx
    from sarx import _ffi, cluster as K
    md, link = 700, (3, 5)
    counts = [300, 0, 700, 1, 65]
    frames = [ref.make_reports(random_cells(c, 20 + f, side=96), seed=f) for f, c in enumerate(counts)]
    raws = [ref.slot_bytes(fr, md) for fr in frames]
    one = [device_step(r, link, 1, md) for r in raws]
    two = [device_step(r, link, 1, md) for r in raws]
    for a, b in zip(one, two):
        assert np.array_equal(a.slot, b.slot) and np.array_equal(a.plots_raw, b.plots_raw) and np.array_equal(a.labels, b.labels)
    # the five slots 24 bytes apart from back to back, the plot records 64: records behind the reports are skipped
    ctx = sarx.default_context()
    cp = sarx.ClusterParams(link=link).c_params(md)
    slot, rec = 16 + 48 * md, 64 * md
    stack = np.zeros((5, slot + 24), np.uint8)
    for f, r in enumerate(raws):
        stack[f, :slot] = r
    bufs = [ctx.to_device(stack), ctx.alloc(5 * (slot + 24)), ctx.alloc(5 * (rec + 64)), ctx.alloc(5 * md * 4)]
    try:
        d_in, d_out, d_plots, d_labels = bufs
        for b in bufs[1:]:
            _ffi.check(ctx.lib.sarx_memset(ctx.h, b.ptr, 0xFF, b.nbytes), ctx.h)
        K.enqueue_run(ctx, cp, d_in.ptr, slot + 24, d_out.ptr, slot + 24, 5, d_plots.ptr, rec + 64, d_labels.ptr)
        out = d_out.download(np.uint8, (5, slot + 24)).copy()
        plots = d_plots.download(np.uint8, (5, rec + 64)).copy()
        labels = d_labels.download(np.int32, (5, md)).copy()
        K.enqueue_run(ctx, cp, d_in.ptr, slot + 24, d_out.ptr, slot + 24, 0, d_plots.ptr, rec + 64, d_labels.ptr)     # no frame: no launch
        ctx.sync()
    finally:
        for b in bufs:
            b.release()
    for f in range(5):
        assert np.array_equal(out[f, :slot], one[f].slot) and (out[f, slot:] == 0xFF).all(), f
        assert np.array_equal(plots[f, :rec], one[f].plots_raw) and (plots[f, rec:] == 0xFF).all(), f
        assert np.array_equal(labels[f], one[f].labels), f
        ref.compare(ref.cluster(frames[f], 3, 5, 1, max_detections=md), out[f, :16], out[f, 16:], plots[f], labels[f])


def test_arguments_the_header_forbids():
    """Past the context check, on the device: overlap, strides, alignment - SARX_ERR_INVALID and nothing launched."""
    import ctypes as C
    import sarx
    ctx = sarx.default_context()
    md = 8
    cp = sarx.ClusterParams().c_params(md)
    slot, rec = 16 + 48 * md, 64 * md
    buf = ctx.alloc(8 * slot + 4 * rec)
    try:
        p = buf.ptr
        step, run = ctx.lib.sarx_cluster_step_dev, ctx.lib.sarx_cluster_run_dev
        bad = [step(ctx.h, C.byref(cp), p, p, None, None), step(ctx.h, C.byref(cp), p, p + slot - 8, None, None),
               step(ctx.h, C.byref(cp), p, p + slot, p + 8, None), step(ctx.h, C.byref(cp), p, p + slot, None, p + slot + 16),
               step(ctx.h, C.byref(cp), p + 4, p + slot, None, None), step(ctx.h, C.byref(cp), None, p + slot, None, None),
               step(ctx.h, C.byref(cp), p, p + slot, None, p + 2 * slot + 2),
               run(ctx.h, C.byref(cp), p, slot - 8, p + 4 * slot, slot, 2, None, 0, None),
               run(ctx.h, C.byref(cp), p, slot + 4, p + 4 * slot, slot, 2, None, 0, None),
               run(ctx.h, C.byref(cp), p, slot, p + 4 * slot, slot, 2, p + 6 * slot, rec - 8, None),
               run(ctx.h, C.byref(cp), p, slot, p + slot, slot, 2, None, 0, None),
               run(ctx.h, C.byref(cp), p, slot, p + 4 * slot, slot, -1, None, 0, None)]
        assert all(rc != 0 for rc in bad), bad
        assert len(ctx.lib.sarx_last_error(ctx.h)) > 10
        assert step(ctx.h, C.byref(cp), p, p + slot, None, None) == 0                  # and the plain call still goes (count 0 or junk: any)
        ctx.sync()
    finally:
        buf.release()


# ---- the Python interface ---------------------------------------------------------------------------------------------------------------
def test_gmti_cluster_takes_every_kind_of_input():
    import sarx
    from sarx import gmti
    det = sarx.GmtiParams(max_detections=256)
    centres = [[50 + 60 * a, 50 + 60 * b] for a in range(3) for b in range(3)]
    rep = ref.make_reports([[ci + 4 * di, cj + 6 * dj] for ci, cj in centres for di in (-1, 0, 1) for dj in (-1, 0, 1)], seed=8)
    want = ref.cluster(rep, 4, 6, 1, max_detections=256)
    ra, ca = 1000.0 + 2.0 * np.arange(512), -100.0 + 0.5 * np.arange(512)
    kw = dict(range_axis=ra, cross_range=ca, wavelength_m=0.03, platform_speed_mps=100.0, lag_s=1e-3, detect=det)
    raw = ref.slot_bytes(rep, 256)
    report = gmti.decode_slot(raw, det, ra, ca, 0.03, 100.0, 1e-3)
    ctx = sarx.default_context()
    held = ctx.to_device(raw)
    try:
        outs = [sarx.gmti_cluster(x, sarx.ClusterParams(link=(4, 6)), **kw) for x in (report, rep.astype(gmti.REPORT_DTYPE), raw, held)]
        many = sarx.gmti_cluster([report, raw, held, ref.make_reports([])], sarx.ClusterParams(link=(4, 6)), **kw)
    finally:
        held.release()
    assert isinstance(many, list) and len(many) == 4 and many[3].n_plots == 0 and many[3].n_reports == 0
    for p in outs + many[:3]:
        assert isinstance(p, sarx.GmtiPlots) and p.n_plots == 9 and p.n_reports == 81 and np.array_equal(p.labels, want.labels[:81])
        assert p.raw.tobytes() == outs[0].raw.tobytes() and p.plots.tobytes() == outs[0].plots.tobytes()
        ref.compare(want, p.raw[:16], p.raw[16:], _records(p), None)
        d = p.detections.detections
        assert len(d) == 9 and np.array_equal(d["interf"], want.reports["interf_re"] + 1j * want.reports["interf_im"])
        np.testing.assert_allclose(d["v_los_mps"], -0.03 * np.angle(d["interf"]) / (4e-3 * np.pi), rtol=1e-15)
        assert np.array_equal(p.plots["extent_az_m"], np.full(9, 4.0)) and np.array_equal(p.plots["extent_rg_m"], np.full(9, 24.0))
    assert sarx.gmti_cluster([], sarx.ClusterParams()) == []
    bare = sarx.gmti_cluster(rep.astype(gmti.REPORT_DTYPE), sarx.ClusterParams(link=(4, 6), min_members=10))     # capacity = the list's length
    assert bare.n_plots == 0 and bare.detections is None and (bare.labels == -1).all() and bare.n_reports == 81


def _records(p):
    from sarx import cluster as K
    rec = np.zeros(p.n_plots, K.PLOT_DTYPE)
    for name in K.PLOT_DTYPE.names:
        rec[name] = p.plots[name]
    return rec


# ---- end to end: the C3 batch -------------------------------------------------------------------------------------------------------------
LINK = (8, 32)


@pytest.fixture(scope="module")
def c3():
    """The 1024-pixel C3 batch of tests/test_gpu_track.py three times: as it always was, with cluster=None said aloud, and with
    cluster= and track=."""
    import sarx
    from sarx.batch import TwoChannelBatch
    ctx = sarx.default_context()
    n, frames = 1024, 6
    det = sarx.GmtiParams(guard=(3, 16), train=(8, 8), pfa=1e-6, max_detections=16384)
    kw = dict(stack="detections", scene="c3", scene_scale=0.25, detect=det)
    out = dict(det=det, frames=frames)
    b = TwoChannelBatch(ctx, n, frames, **kw)
    b.run()
    ctx.sync()
    out["plain"] = b.stack().copy().view(np.uint8)
    out["plain_slot_bytes"] = b.slot_bytes
    out["reports"] = [b.detections(f) for f in range(frames)]
    out["axes"] = b._lane_state[0]["plan"].axes()
    out["radar"] = (b.focus_args[0], b.focus_args[5], 1.0 / b.focus_args[4])
    b.close()
    b = TwoChannelBatch(ctx, n, frames, cluster=None, **kw)
    b.run()
    ctx.sync()
    out["none"] = b.stack().copy().view(np.uint8)
    b.close()
    b = TwoChannelBatch(ctx, n, frames, cluster=sarx.ClusterParams(link=LINK), track=sarx.TrackParams(confirm=(2, 3), max_tracks=16384), **kw)
    b.run()
    ctx.sync()
    out["clustered"] = b.stack().copy().view(np.uint8)
    out["clustered_slot_bytes"], out["plots_offset"] = b.slot_bytes, b.plots_offset
    out["plots"] = [b.plots(f) for f in range(frames)]
    out["decoded"] = [b.detections(f) for f in range(frames)]
    out["tracks"] = b.tracks()
    b.close()
    return out


def test_batch_without_cluster_is_what_it_was(c3):
    assert c3["plain_slot_bytes"] == 16 + 48 * 16384 and np.array_equal(c3["plain"], c3["none"])
    assert c3["clustered_slot_bytes"] == 16 + (48 + 64) * 16384 and c3["plots_offset"] == 16 + 48 * 16384


def test_batch_plots_equal_gmti_cluster_and_the_restatement(c3):
    import sarx
    det, frames = c3["det"], c3["frames"]
    ra, ca = c3["axes"]
    lam, v, lag = c3["radar"]
    alone = sarx.gmti_cluster(c3["reports"], sarx.ClusterParams(link=LINK), detect=det)          # one launch for the six lists
    n_reports, n_plots = [], []
    for f in range(frames):
        slot = c3["clustered"][f]
        k = alone[f].n_plots
        n_reports.append(len(c3["reports"][f]))
        n_plots.append(k)
        assert slot[:16 + 48 * k].tobytes() == alone[f].raw.tobytes(), f
        off = c3["plots_offset"]
        assert slot[off:off + 64 * k].tobytes() == alone[f].plots.tobytes(), f
        assert not slot[16 + 48 * k:off].any() and not slot[off + 64 * k:].any()               # no stale bytes in the slot
        rep = c3["plain"][f][16:16 + 48 * n_reports[f]].view(ref.REPORT_DTYPE)
        want = ref.cluster(rep, LINK[0], LINK[1], 1, max_detections=16384)
        ref.compare(want, slot[:16], slot[16:], slot[off:], None)
        assert np.array_equal(alone[f].labels, want.labels[:n_reports[f]])
        p = c3["plots"][f]
        assert p.n_plots == k and p.n_reports == n_reports[f] and p.labels is None
        assert len(c3["decoded"][f]) == k and np.array_equal(c3["decoded"][f].detections["interf"], p.detections.detections["interf"])
        assert k < n_reports[f]
    t = c3["tracks"]
    print("C3 1024, link", LINK, ": reports per frame", n_reports, "plots per frame", n_plots)
    print("tracks on plots: live", t.n_live, "confirmed", t.n_confirmed, "(on the raw reports: 268 live, 246 confirmed)")
    assert t.n_confirmed >= 1
