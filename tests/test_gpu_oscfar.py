"""The ordered-statistic CFAR on the GPU (sarx.gmti_detect(method="os"), focus_ati_dpca(detect=...), TwoChannelBatch; csrc/oscfar.hip)
against the NumPy restatement of its semantics (tests/_oscfar_numpy.py).  The decision is an integer count of exact fp64
comparisons and the level an element of the plane squared, so the reported (i, j) lists, `power` and `mean` (= the level) must be
bit-identical to the restatement: there is no band."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmti_numpy as ca_ref  # noqa: E402
import _oscfar_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu

LAM, V, LAG = 0.031, 7500.0, 1.0 / 6000.0
SHAPES = [(64, 64), (33, 65), (96, 80), (1, 200), (200, 1)]             # 33 x 65: one row and one column past a tile
WINDOWS = [((2, 2), (8, 8)), ((0, 0), (1, 1)), ((1, 3), (31, 29)), ((4, 0), (0, 12)), ((0, 5), (9, 0))]
RANKS = ["one", "full", "three-quarters"]
PFA = 1e-3


def _rank(name, nf):
    return {"one": 1, "full": nf, "three-quarters": (3 * nf) // 4, "half": nf // 2}[name]


@functools.lru_cache(maxsize=None)
def _plane(shape, seed=None):
    m = ref.speckle_plane(shape, shape[0] * 1000 + shape[1] if seed is None else seed)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _images(shape):
    rng = np.random.default_rng(shape[0] + 3 * shape[1])
    s1 = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    s2 = (s1 * np.exp(-0.3j)).astype(np.complex64)
    return s1, s2


def _detect(m, **kw):
    import sarx
    n_az, n_rg = m.shape
    s1, s2 = _images(m.shape)
    kw.setdefault("max_detections", 65536)
    return sarx.gmti_detect(s1.T, s2.T, np.arange(float(n_rg)), np.arange(float(n_az)), wavelength_m=LAM, platform_speed_mps=V, lag_s=LAG,
                            dpca_mag=np.asarray(m).T, method="os", **kw)


def _assert_identical(rep, o):
    d = rep.detections
    cells = list(zip(d["i"].tolist(), d["j"].tolist()))
    assert cells == o["cells"], (len(cells), len(o["cells"]), sorted(set(cells) ^ set(o["cells"]))[:10])
    assert d["power"].tobytes() == np.asarray(o["power"], np.float64).tobytes()
    assert d["mean"].tobytes() == np.asarray(o["level"], np.float64).tobytes()


def _raw(m, cp, max_det):
    """The two launches through the C ABI with the given sarx_oscfar_params: header fields and the report array."""
    import sarx
    from sarx import gmti as G
    from sarx._ffi import check
    ctx = sarx.default_context()
    n_az, n_rg = m.shape
    s1, s2 = _images(m.shape)
    bufs = [ctx.to_device(np.ascontiguousarray(x)) for x in (m, s1, s2)] + [ctx.alloc(G.HEADER_BYTES + 48 * max_det)]
    try:
        slot = bufs[3].ptr
        check(ctx.lib.sarx_gmti_oscfar_dev(ctx.h, bufs[0].ptr, n_az, n_rg, C.byref(cp), slot + G.HEADER_BYTES, slot), ctx.h)
        check(ctx.lib.sarx_gmti_refine_dev(ctx.h, bufs[1].ptr, bufs[2].ptr, n_az, n_rg, 0.0, slot + G.HEADER_BYTES, slot, max_det), ctx.h)
        raw = G.fetch_slot(ctx, slot, max_det)
    finally:
        for b in bufs:
            b.release()
    count, overflow = (int(x) for x in raw[:8].view("<u4"))
    return count, overflow, raw[G.HEADER_BYTES:].view(G.REPORT_DTYPE)


@pytest.mark.parametrize("rank_name", RANKS)
@pytest.mark.parametrize("guard,train", WINDOWS, ids=[f"g{g[0]}.{g[1]}-t{t[0]}.{t[1]}" for g, t in WINDOWS])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_bit_identical_to_the_restatement(shape, guard, train, rank_name):
    from sarx.gmti import os_cfar_alpha
    nf = ref.n_full(guard, train)
    rank = _rank(rank_name, nf)
    m = _plane(shape)
    rep = _detect(m, guard=guard, train=train, pfa=PFA, os_rank=rank)
    assert (rep.method, rep.rank, rep.n_full) == ("os", rank, nf)
    assert rep.alpha == os_cfar_alpha(PFA, nf, rank)
    o = ref.oscfar(m, guard, train, alpha=rep.alpha, rank=rank)
    print(f"{shape} guard {guard} train {train} rank {rank}/{nf}: {len(o['cells'])} reports, {int(o['tested'].sum())} cells tested")
    _assert_identical(rep, o)
    if min(shape) >= 33:                                                  # a window wider than a thin plane leaves nothing to test
        assert o["tested"].any()
        if rank_name != "full":
            assert len(o["cells"]) >= 1


LADDER = (8, 9, 16, 17)                   # outer half-widths at the steps of the halo ladder: HA, HR = 8, 16, 16, 32
LADDER_GUARD = (2, 2)


@pytest.mark.parametrize("outer_rg", LADDER)
@pytest.mark.parametrize("outer_az", LADDER)
def test_bit_identical_on_every_rung_of_the_halo_ladder(outer_az, outer_rg):
    """The sixteen windows reach all nine (HA, HR) instantiations of the OS kernel, on the plane that is past one tile in both
    directions, at the default rank."""
    from sarx.gmti import os_cfar_alpha
    train = (outer_az - LADDER_GUARD[0], outer_rg - LADDER_GUARD[1])
    nf, rank = ref.n_full(LADDER_GUARD, train), ref.default_rank(LADDER_GUARD, train)
    m = _plane((96, 80))
    rep = _detect(m, guard=LADDER_GUARD, train=train, pfa=PFA)
    assert (rep.method, rep.rank, rep.n_full) == ("os", rank, nf)
    assert rep.alpha == os_cfar_alpha(PFA, nf, rank)
    o = ref.oscfar(m, LADDER_GUARD, train, alpha=rep.alpha, rank=rep.rank)
    assert len(o["cells"]) >= 1                                           # a case cannot pass by detecting nothing
    _assert_identical(rep, o)


@pytest.mark.parametrize("shape,guard,train", [((1, 200), (0, 5), (0, 12)), ((200, 1), (4, 0), (9, 0)), ((33, 65), (2, 2), (8, 8))],
                         ids=["1x200", "200x1", "33x65"])
def test_thin_planes_and_borders_with_min_train_one(shape, guard, train):
    """min_train = 1 through the C ABI: every cell with a training cell is tested, so the corners and borders (k scaled to a small
    N) and the planes of one row or column decide something."""
    import sarx
    nf = ref.n_full(guard, train)
    m = _plane(shape)
    for rank in (1, (3 * nf) // 4, nf):
        cp = sarx.GmtiParams(guard, train, PFA, method="os", os_rank=rank, max_detections=4096).c_params()
        cp.base.min_train = 1
        count, overflow, rep = _raw(m, cp, 4096)
        o = ref.oscfar(m, guard, train, alpha=cp.base.alpha, rank=rank, min_train=1)
        assert o["tested"].all() and not overflow and count == len(o["cells"])
        assert list(zip(rep["i"].tolist(), rep["j"].tolist())) == o["cells"]
        assert rep["power"].tobytes() == o["power"].tobytes() and rep["mean"].tobytes() == o["level"].tobytes()
        border = [c for c in o["cells"] if c[0] in (0, shape[0] - 1) or c[1] in (0, shape[1] - 1)]
        print(f"{shape} rank {rank}/{nf}: {count} reports, {len(border)} on the border")
        if rank < nf:
            assert border


def test_1000x777():
    m = _plane((1000, 777))
    rep = _detect(m, pfa=1e-4)
    o = ref.oscfar(m, alpha=rep.alpha, rank=312)
    print(f"1000 x 777: {len(o['cells'])} reports")
    assert len(o["cells"]) > 100
    _assert_identical(rep, o)


@pytest.mark.parametrize("rank_name", ["one", "half"])
def test_quantised_plane_exercises_the_strict_compare(rank_name):
    """m in {1, 2, 4}, alpha = 4.0: alpha * P_t == P exactly wherever a cell of m = 2 meets a level of 1."""
    guard, train = (1, 1), (4, 4)
    nf = ref.n_full(guard, train)
    rank = _rank(rank_name, nf)
    m = ref.quantised_plane((70, 70), 5)
    every = ref.oscfar(m, guard, train, alpha=4.0, rank=rank, every_cell=True)
    ties = every["tested"] & (4.0 * every["level_map"] == every["p"])
    flips = ties & every["peak"]                                          # cells a non-strict compare would report
    print(f"rank {rank}/{nf}: {int(ties.sum())} tested cells with alpha x_(k) == P, {int(flips.sum())} of them peaks, "
          f"{len(every['cells'])} reports")
    assert ties.sum() >= 100 and flips.sum() >= 10 and len(every["cells"]) >= 10
    assert not (every["detected"] & ties).any()
    rep = _detect(m, guard=guard, train=train, alpha=4.0, os_rank=rank)
    assert rep.alpha == 4.0
    _assert_identical(rep, every)


def test_all_zero_plane_and_a_plane_smaller_than_the_guard_box():
    z = np.zeros((70, 130), np.float32)
    assert _detect(z).n_found == 0
    m = _plane((3, 3), 9)
    rep = _detect(m, guard=(2, 2), train=(1, 1))                          # guard box 5 x 5 over a 3 x 3 plane: no training cell at all
    o = ref.oscfar(m, (2, 2), (1, 1), alpha=rep.alpha)
    assert not o["tested"].any() and o["n_train"].max() == 0 and rep.n_found == 0


def test_masking_scene_os_reports_all_eight_ca_only_the_strong_four():
    import sarx
    m = ref.masking_scene()
    s1, s2 = _images(m.shape)
    ax = np.arange(96.0)
    kw = dict(wavelength_m=LAM, platform_speed_mps=V, lag_s=LAG, dpca_mag=m.T, pfa=1e-6)
    os_ = sarx.gmti_detect(s1.T, s2.T, ax, ax, method="os", **kw)
    ca = sarx.gmti_detect(s1.T, s2.T, ax, ax, method="ca", **kw)
    cells = lambda r: list(zip(r.detections["i"].tolist(), r.detections["j"].tolist()))
    assert cells(os_) == sorted(ref.MASKING_CELLS)
    assert cells(ca) == sorted(c for c, db in zip(ref.MASKING_CELLS, ref.MASKING_DB) if db == 40)
    assert cells(ca) == ca_ref.cfar(m, pfa=1e-6)["cells"]
    assert (os_.method, os_.rank, ca.method, ca.rank) == ("os", 312, "ca", None)
    _assert_identical(os_, ref.oscfar(m, alpha=os_.alpha, rank=312))
    # snr_db is power over the level the cell was held against
    d = os_.detections
    np.testing.assert_array_equal(d["snr_db"], 10.0 * np.log10(d["power"] / d["mean"]))


def test_two_runs_give_identical_bytes_and_overflow_raises():
    import sarx
    m = _plane((1000, 777))
    a, b = _detect(m, pfa=1e-3), _detect(m, pfa=1e-3)
    assert a.n_found > 100 and a.detections.tobytes() == b.detections.tobytes()
    o = ref.oscfar(m, alpha=a.alpha, rank=312)
    assert a.n_found == len(o["cells"])
    with pytest.raises(sarx.GmtiOverflowError) as e:
        _detect(m, pfa=1e-3, max_detections=len(o["cells"]) - 1)
    assert e.value.count == len(o["cells"])
    c = _detect(m, pfa=1e-3, max_detections=len(o["cells"]))              # exactly full: no overflow
    assert c.detections.tobytes() == a.detections.tobytes()


@pytest.mark.parametrize("n_az,n_rg", [(256, 256), (200, 240)])
def test_fused_equals_standalone(n_az, n_rg):
    import sarx
    from oracle import csa_oracle as orc
    (r1, r2), k = orc.point_scene(n_az, n_rg, seed=5, clutter_db=-25.0, two_channel=True)
    args = orc.focus_args(k)
    params = sarx.GmtiParams(pfa=1e-3, max_detections=8192, method="os")
    res = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, detect=params, cal_phase=0.2, return_slc2=False)
    full = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, cal_phase=0.2)
    alone = sarx.gmti_detect(full["slc1"], full["slc2"], full["range_axis"], full["cross_range"], wavelength_m=args[0],
                             platform_speed_mps=args[5], lag_s=1.0 / args[4], pfa=1e-3, cal_phase=0.2, max_detections=8192, method="os")
    a, b = res["detections"], alone
    assert len(a) > 3 and (a.method, a.rank) == ("os", 312) == (b.method, b.rank)
    assert a.detections.tobytes() == b.detections.tobytes()
    ca = sarx.focus_ati_dpca(r1, r2, *args, pulse_shift=False, detect=sarx.GmtiParams(pfa=1e-3, max_detections=8192), cal_phase=0.2)
    assert ca["detections"].method == "ca" and ca["detections"].rank is None


def test_batch_detections_with_the_tracker():
    """TwoChannelBatch(stack="detections", detect=GmtiParams(method="os"), track=...) at 1024: every frame's list is what
    gmti_detect reports on the frame's DPCA plane (taken from a products batch), frame 0's is the restatement's, and the tracker
    runs on the slots."""
    import sarx
    from sarx.batch import TwoChannelBatch
    ctx = sarx.default_context()
    n, frames = 1024, 3
    det = sarx.GmtiParams(pfa=1e-6, max_detections=16384, method="os")
    b = TwoChannelBatch(ctx, n, frames, stack="detections", scene="c3", scene_scale=0.25, detect=det,
                        track=sarx.TrackParams(confirm=(2, 3), max_tracks=16384))
    assert b.slot_bytes == 16 + 48 * 16384
    b.run()
    ctx.sync()
    reports = [b.detections(f) for f in range(frames)]
    tracks = b.tracks()
    b.close()
    bp = TwoChannelBatch(ctx, n, frames, stack="products", scene="c3", scene_scale=0.25)
    bp.run()
    ctx.sync()
    st = bp.stack()
    bp.close()
    zeros = np.zeros((n, n), np.complex64)
    ax = np.arange(float(n))
    for f in range(frames):
        alone = sarx.gmti_detect(zeros, zeros, ax, ax, wavelength_m=LAM, platform_speed_mps=V, lag_s=LAG, pfa=1e-6, max_detections=16384,
                                 dpca_mag=st[f, 2].T, method="os")
        for key in ("i", "j", "power", "mean"):
            assert reports[f].detections[key].tobytes() == alone.detections[key].tobytes(), (f, key)
        assert (reports[f].method, reports[f].rank) == ("os", 312) and 1 <= reports[f].n_found < 16384
    _assert_identical(reports[0], ref.oscfar(st[0, 2], alpha=reports[0].alpha, rank=312))
    print("reports per frame", [len(r) for r in reports], "live", tracks.n_live, "confirmed", tracks.n_confirmed)
    assert tracks.n_live >= 1 and tracks.assoc.shape[0] == frames


def test_refusals_leave_a_poisoned_slot_untouched():
    import sarx
    from sarx import gmti as G
    from sarx._ffi import check
    ctx = sarx.default_context()
    m = _plane((64, 64))
    d_m, slot = ctx.to_device(np.ascontiguousarray(m)), ctx.alloc(G.HEADER_BYTES + 48 * 64)
    good = lambda: sarx.GmtiParams(method="os", max_detections=64).c_params()

    def edit(**kw):
        cp = good()
        for k, v in kw.items():
            setattr(cp.base if hasattr(cp.base, k) else cp, k, v)
        return cp

    try:
        check(ctx.lib.sarx_memset(ctx.h, slot.ptr, 0xFF, slot.nbytes), ctx.h)
        rep, hdr = slot.ptr + G.HEADER_BYTES, slot.ptr
        call = lambda cp, mag=d_m.ptr, n_az=64, n_rg=64, rep=rep, hdr=hdr: ctx.lib.sarx_gmti_oscfar_dev(
            ctx.h, mag, n_az, n_rg, C.byref(cp) if cp is not None else None, rep, hdr)
        for cp in (edit(rank=0), edit(rank=-3), edit(rank=417), edit(flags=1), edit(alpha=0.0), edit(alpha=float("nan")), edit(guard_az=-1),
                   edit(min_train=0), edit(max_detections=0), edit(train_az=0, train_rg=0)):
            assert call(cp) == -1                                         # SARX_ERR_INVALID
            assert len(ctx.lib.sarx_last_error(ctx.h)) > 10
        assert call(edit(train_az=31)) not in (0, -1)                     # SARX_ERR_UNSUPPORTED
        assert b"exceed" in ctx.lib.sarx_last_error(ctx.h)                # the CA launch's own words reach the context
        assert call(None) == -1 and call(good(), mag=None) == -1 and call(good(), rep=None) == -1 and call(good(), hdr=None) == -1
        assert call(good(), n_az=0) == -1 and call(good(), n_rg=-1) == -1
        assert call(good(), rep=rep + 4) == -1 and call(good(), hdr=hdr + 2) == -1 and call(good(), mag=d_m.ptr + 2) == -1
        ctx.sync()
        raw = np.empty(slot.nbytes, np.uint8)
        check(ctx.lib.sarx_memcpy_d2h(ctx.h, raw.ctypes.data, slot.ptr, slot.nbytes), ctx.h)
        assert (raw == 0xFF).all()
        assert call(good()) == 0                                          # and the same arguments, valid, run
        ctx.sync()
    finally:
        d_m.release()
        slot.release()
