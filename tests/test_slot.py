"""CPU checks of the host side of the GMTI slot (sarx/slot.py) and of the one chain (sarx.gmti.enqueue_chain): the byte round trip,
the overflow rule of every reader as slot.py's table states it, the chain's call sequence and buffer roles against a recording
stand-in for the context, and the shared guard / train window check."""
import ctypes as C

import numpy as np
import pytest

import sarx
from sarx import atigate, cluster, gmti, slot, track

MD = 8


def _reports(n, seed=3):
    rng = np.random.default_rng(seed)
    rep = np.zeros(n, slot.REPORT_DTYPE)
    rep["i"], rep["j"] = np.arange(n), rng.integers(0, 32, n)
    for k in ("power", "mean", "interf_re", "interf_im", "mag1", "mag2"):
        rep[k] = rng.uniform(1.0, 2.0, n)
    return rep


def _with_header(count, overflow):
    """A full slot of MD reports whose header claims (count, overflow)."""
    raw = slot.encode(_reports(MD), MD)
    raw[:8].view("<u4")[:] = (count, overflow)
    return raw


HEADERS = ((MD, 0), (MD + 1, 0), (MD + 1, 1))


def test_round_trip_padding_and_limits():
    assert slot.encode is track.encode_slot and slot.fetch is gmti.fetch_slot and slot.decode is gmti.decode_slot
    assert slot.count_of is cluster.count_of and slot.GmtiOverflowError is gmti.GmtiOverflowError is sarx.GmtiOverflowError
    assert gmti.HEADER_BYTES == slot.HEADER_BYTES == 16 and gmti.REPORT_DTYPE is slot.REPORT_DTYPE
    assert slot.slot_bytes(MD) == cluster.slot_bytes(MD) == atigate.slot_bytes(MD) == track.TrackParams(max_detections=MD).slot_bytes() \
        == gmti.GmtiParams(max_detections=MD).slot_bytes() == 16 + 48 * MD
    for n in (0, 1, MD):
        rep = _reports(n)
        raw = slot.encode(rep, MD)
        assert raw.dtype == np.uint8 and raw.shape == (16 + 48 * MD,)
        assert slot.header(raw) == (n, 0) and slot.count_of(raw) == slot.count_of(rep) == n
        got = slot.reports(raw)
        assert got.dtype == slot.REPORT_DTYPE and got.tobytes() == rep.tobytes()
        assert slot.reports(raw, 0).size == 0 and not raw[16 + 48 * n:].any()
    raw = slot.encode(_reports(3), MD)
    assert np.array_equal(slot.encode(raw[:16 + 48 * 3], MD), raw)                # a trimmed slot is padded to the full size
    with pytest.raises(slot.GmtiOverflowError) as e:
        slot.encode(_reports(MD + 1), MD)
    assert (e.value.count, e.value.max_detections) == (MD + 1, MD)
    for bad in (raw[:15], np.zeros(16 + 48 * MD + 1, np.uint8)):
        with pytest.raises(ValueError, match="a raw slot is a header and at most max_detections reports"):
            slot.encode(bad, MD)


def test_stage_capacity_items_and_messages():
    class Dev:
        ptr = 4096
    rep = _reports(3)
    md, stack, on_device = slot.stage(rep)
    assert md == 3 and on_device == [] and np.array_equal(stack, slot.encode(rep, 3)[None])
    md, stack, on_device = slot.stage([rep, Dev(), slot.encode(rep, MD)[:16 + 48 * 3]], max_detections=MD)
    assert md == MD and on_device == [(1, 4096)] and stack.shape == (3, 16 + 48 * MD)
    assert np.array_equal(stack[0], stack[2]) and not stack[1].any()
    assert slot.stage([], None, None)[0] == 1 and slot.stage(rep, gmti.GmtiParams(max_detections=64), 5)[0] == 64
    with pytest.raises(ValueError, match=r"device slots need detect= or max_detections= \(their capacity\)"):
        slot.stage([rep, Dev()])
    with pytest.raises(ValueError, match=r"device slots need detect= or max_detections= \(their capacity\)"):
        slot.stage(Dev())
    with pytest.raises(ValueError, match=r"a device slot needs detect= or max_detections= \(its capacity\)"):
        slot.stage(Dev(), single=True)


class _HostCtx:
    """A context whose "device" is host memory: sarx_memcpy_d2h copies from the address it is given."""
    h = None

    class lib:
        @staticmethod
        def sarx_memcpy_d2h(h, dst, src, n):
            C.memmove(dst, src, n)
            return 0


# slot.py's table, row by row: does the reader raise for (count, overflow) = (md, 0), (md + 1, 0), (md + 1, 1)?
STRICT, OVERFLOW_ONLY, NEVER = (False, True, True), (False, False, True), (False, False, False)


@pytest.mark.parametrize("strict, want", [(True, STRICT), (False, OVERFLOW_ONLY)])
def test_overflow_helper(strict, want):
    for (count, overflow), raises in zip(HEADERS, want):
        if raises:
            with pytest.raises(slot.GmtiOverflowError) as e:
                slot.raise_if_overflowed(count, overflow, MD, strict=strict)
            assert (e.value.count, e.value.max_detections) == (count, MD)
        else:
            assert slot.raise_if_overflowed(count, overflow, MD, strict=strict) == count


def _decode(raw):
    return gmti.decode_slot(raw, gmti.GmtiParams(max_detections=MD), np.arange(32.0), np.arange(float(MD)), 0.03, 100.0, 1e-3)


def _plots(raw):
    return cluster.GmtiPlots(raw, np.zeros((MD + 1) * cluster.PLOT_DTYPE.itemsize, np.uint8), None, MD,
                             detect=gmti.GmtiParams(max_detections=MD))


def _fetch(raw):
    return slot.fetch(_HostCtx, raw.ctypes.data, MD)


def _fetch_gate(raw):
    return atigate.fetch_gate(_HostCtx, raw.ctypes.data, np.zeros((MD + 1) * atigate.GATE_DTYPE.itemsize, np.uint8).ctypes.data)


def _fetch_plots(raw):
    rec = np.zeros((MD + 1) * cluster.PLOT_DTYPE.itemsize, np.uint8)
    return cluster.fetch_plots(_HostCtx, raw.ctypes.data, rec.ctypes.data, None, MD, n_reports=MD)


@pytest.mark.parametrize("site, want", [(_decode, STRICT), (_plots, OVERFLOW_ONLY), (_fetch_plots, OVERFLOW_ONLY), (_fetch, NEVER),
                                        (_fetch_gate, NEVER), (slot.count_of, NEVER), (lambda raw: track._slot_ij(raw, MD), NEVER)])
def test_overflow_rule_site_by_site(site, want):
    for (count, overflow), raises in zip(HEADERS, want):
        raw = _with_header(count, overflow)
        if raises:
            with pytest.raises(slot.GmtiOverflowError) as e:
                site(raw)
            assert e.value.count == count and e.value.max_detections == MD
        else:
            site(raw)


def test_readers_that_do_not_raise_clamp_or_take_the_count_as_it_stands():
    for count, overflow in HEADERS:
        raw = _with_header(count, overflow)
        assert slot.count_of(raw) == count                                        # the count as it stands
        assert track._slot_ij(raw, MD).shape == (MD, 2)                           # clamp
        got = _fetch(raw)
        assert got.size == 16 + 48 * MD and slot.header(got) == (count, overflow) and np.array_equal(got, raw)
        assert len(_fetch_gate(raw)) == (0 if overflow else count)                # no records for an overflowed list
    assert len(_decode(_with_header(MD, 0))) == MD and _plots(_with_header(MD + 1, 0)).n_plots == MD + 1


# ---- the chain -------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for a Context: every ctx.lib.sarx_* call is appended as (name, args) and answers SARX_OK."""

    def __init__(self):
        self.h, self.calls = object(), []
        outer = self

        class Lib:
            def __getattr__(self, name):
                return lambda *args: outer.calls.append((name, args)) or 0
        self.lib = Lib()


MAG, S1, S2, N, CAP = 0x1000, 0x2000, 0x3000, 64, 16
SLOTS, STATS, PLOTS, LABELS = (0x10000, 0x20000, 0x30000), 0x40000, 0x50000, 0x60000


@pytest.mark.parametrize("method", ["ca", "os"])
@pytest.mark.parametrize("with_cluster", [False, True])
@pytest.mark.parametrize("with_gate", [False, True])
@pytest.mark.parametrize("extras", [True, False])          # False: the batch's hand-off, no statistics and no labels are kept
def test_chain_call_sequence_and_buffer_roles(with_gate, with_cluster, method, extras):
    ctx = _Recorder()
    params = gmti.GmtiParams(max_detections=CAP, method=method)
    gate = (sarx.AtiGateParams().c_params(CAP), STATS if extras else None) if with_gate else None
    plots = (sarx.ClusterParams().c_params(CAP), PLOTS, LABELS if extras else None) if with_cluster else None
    slots = SLOTS[:1 + with_gate + with_cluster]
    last = gmti.enqueue_chain(ctx, MAG, S1, S2, N, N, params, 0.25, slots, gate, plots)
    assert last == slots[-1]                                                      # what refocus, tracker or fetch read next
    names = [name for name, _ in ctx.calls]
    assert names == ["sarx_gmti_cfar_dev" if method == "ca" else "sarx_gmti_oscfar_dev", "sarx_gmti_refine_dev"] + \
        ["sarx_atigate_step_dev"] * with_gate + ["sarx_cluster_step_dev"] * with_cluster
    calls = iter(ctx.calls)
    h, mag, n_az, n_rg, cp, rep, hdr = next(calls)[1]                             # CFAR into the first slot: reports behind the header
    assert (h, mag, n_az, n_rg, rep, hdr) == (ctx.h, MAG, N, N, slots[0] + 16, slots[0])
    h, s1, s2, n_az, n_rg, cal, rep, hdr, md = next(calls)[1]                     # refine in place
    assert (h, s1, s2, n_az, n_rg, cal, rep, hdr, md) == (ctx.h, S1, S2, N, N, 0.25, slots[0] + 16, slots[0], CAP)
    cur = slots[0]
    if with_gate:                                                                 # the gate reads the detector's slot, writes the next
        h, cp, s1, s2, n_az, n_rg, src, dst, stats = next(calls)[1]
        assert (h, s1, s2, n_az, n_rg, src, dst, stats) == (ctx.h, S1, S2, N, N, cur, slots[1], STATS if extras else None)
        cur = slots[1]
    if with_cluster:                                                              # the cluster reads the gated slot if there is one
        h, cp, src, dst, rec, labels = next(calls)[1]
        assert (h, src, dst, rec, labels) == (ctx.h, cur, slots[-1], PLOTS, LABELS if extras else None)
    assert next(calls, None) is None


# ---- the window check ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guard, train, message", [
    ((-1, 2), (8, 8), "guard and train half-widths must be >= 0"), ((2, 2), (8, -1), "guard and train half-widths must be >= 0"),
    ((2, 2), (31, 8), r"guard \+ train half-widths \(33, 10\) exceed 32"), ((4, 2), (29, 8), r"guard \+ train half-widths \(33, 10\) exceed 32"),
    ((2, 3), (8, 30), r"guard \+ train half-widths \(10, 33\) exceed 32"), ((2, 2), (0, 0), "the training set is empty")])
def test_window_check_is_shared(guard, train, message):
    for check in (lambda: gmti.window(guard, train), gmti.GmtiParams(guard=guard, train=train).resolved,
                  sarx.AtiGateParams(guard=guard, train=train).check):
        with pytest.raises(ValueError, match=message):
            check()


@pytest.mark.parametrize("guard, train", [((2, 2), (8, 8)), ((0, 0), (1, 0)), ((0, 3), (32, 29))])
def test_n_full_agrees(guard, train):
    (ga, gr), (ta, tr) = guard, train
    nf = (2 * (ga + ta) + 1) * (2 * (gr + tr) + 1) - (2 * ga + 1) * (2 * gr + 1)
    assert gmti.n_full(guard, train) == nf and gmti.window(guard, train) == (ga, gr, ta, tr, nf)
    assert gmti.GmtiParams(guard=guard, train=train).resolved()[:5] == (ga, gr, ta, tr, nf)
    gate = sarx.AtiGateParams(guard=guard, train=train, looks=(0, 0))
    assert gate.check()[:4] == (ga, gr, ta, tr) and gate.c_params(CAP).min_train == (nf + 1) // 2
