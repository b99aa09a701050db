"""Guard bands and poison around the two device entry points of include/sarx_cluster.h (tests/_guard.py, the protocol of
tests/test_gpu_guard.py): every device argument is a GuardedBuffer, each case runs once with every output poisoned (0xFF) and once
zeroed; the promised bytes - the header, the n_plots reports and records, every label - must be bit-identical in both runs and
equal to the restatement, every other output byte still poison, every zone clean and the input slot unchanged.  Payloads sit 0 and
8 bytes off a 16-byte boundary; n = 0, 1, 1025 and the overflow, the plot records and the labels each left out in turn."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cluster_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run  # noqa: E402

pytestmark = pytest.mark.gpu

MD, LINK = 1100, (3, 5)          # neither a multiple of a wave nor of the workgroup; the sort runs over 2048


def _frame(kind):
    n = {"empty": 0, "one": 1, "many": 1025, "overflow": 40}[kind]
    flat = np.random.default_rng(n + 1).choice(200 * 200, n, replace=False)
    rep = ref.make_reports(np.stack([flat // 200, flat % 200], axis=1), seed=n)
    kw = dict(overflow=1) if kind == "overflow" else {}
    return ref.slot_bytes(rep, MD, **kw), ref.cluster(rep, LINK[0], LINK[1], 1, max_detections=MD, **kw)


@pytest.fixture(scope="module")
def frames():
    return {k: _frame(k) for k in ("empty", "one", "many", "overflow")}


def _cp():
    import sarx
    return sarx.ClusterParams(link=LINK).c_params(MD)


def _check(want, slot, plots, labels):
    k = want.n_plots
    assert slot[:16].view("<u4").tolist() == want.header.tolist()
    if want.reports is not None:
        assert np.array_equal(slot[16:16 + 48 * k], want.reports.view(np.uint8))
        if plots is not None:
            assert np.array_equal(plots[:64 * k], want.plots.view(np.uint8))
    if labels is not None:
        assert np.array_equal(labels.view(np.int32), want.labels)


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("leave_out", [None, "plots", "labels"])
@pytest.mark.parametrize("kind", ["empty", "one", "many", "overflow"])
def test_step_guard(kind, leave_out, off, frames):
    import sarx
    from sarx import cluster as K
    raw, want = frames[kind]
    ctx, cp = sarx.default_context(), _cp()
    d_in = guarded(ctx, raw, offset=off)
    out = GuardedBuffer(ctx, 16 + 48 * MD, offset=off)
    plots = GuardedBuffer(ctx, 64 * MD, offset=off)
    labels = GuardedBuffer(ctx, 4 * MD, offset=off)
    try:
        k = want.n_plots
        findings, res = guarded_run(
            lambda: K.enqueue_step(ctx, cp, d_in.ptr, out.ptr, None if leave_out == "plots" else plots.ptr,
                                   None if leave_out == "labels" else labels.ptr),
            {"slot_in": (d_in, raw)}, {"slot_out": out, "plots": plots, "labels": labels},
            promised={"slot_out": 16 + 48 * k, "plots": 0 if leave_out == "plots" else 64 * k, "labels": 0 if leave_out == "labels" else 4 * MD},
            sync=ctx.sync)
        assert not findings, findings
        r = res["poisoned"]
        _check(want, r["slot_out"], None if leave_out == "plots" else r["plots"], None if leave_out == "labels" else r["labels"])
    finally:
        for g in (d_in, out, plots, labels):
            g.release()


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("leave_out", [None, "plots", "labels"])
def test_run_guard(leave_out, off, frames):
    import sarx
    from sarx import cluster as K
    order = ["many", "empty", "overflow", "one"]
    slot, rec, pad = 16 + 48 * MD, 64 * MD, 40          # strides 40 bytes longer than the records: the bytes between stay poison
    stack = np.zeros((4, slot + pad), np.uint8)
    for f, kind in enumerate(order):
        stack[f, :slot] = frames[kind][0]
    ctx, cp = sarx.default_context(), _cp()
    d_in = guarded(ctx, stack, offset=off)
    out = GuardedBuffer(ctx, 4 * (slot + pad), offset=off)
    plots = GuardedBuffer(ctx, 4 * (rec + pad), offset=off)
    labels = GuardedBuffer(ctx, 4 * 4 * MD, offset=off)
    try:
        m_out, m_plots = np.zeros(out.nbytes, bool), np.zeros(plots.nbytes, bool)
        for f, kind in enumerate(order):
            k = frames[kind][1].n_plots
            m_out[f * (slot + pad):f * (slot + pad) + 16 + 48 * k] = True
            if leave_out != "plots":
                m_plots[f * (rec + pad):f * (rec + pad) + 64 * k] = True
        findings, res = guarded_run(
            lambda: K.enqueue_run(ctx, cp, d_in.ptr, slot + pad, out.ptr, slot + pad, 4, None if leave_out == "plots" else plots.ptr,
                                  rec + pad, None if leave_out == "labels" else labels.ptr),
            {"stack_in": (d_in, stack)}, {"stack_out": out, "plots": plots, "labels": labels},
            promised={"stack_out": m_out, "plots": m_plots, "labels": 0 if leave_out == "labels" else 16 * MD}, sync=ctx.sync)
        assert not findings, findings
        r = res["poisoned"]
        for f, kind in enumerate(order):
            _check(frames[kind][1], r["stack_out"][f * (slot + pad):][:slot], None if leave_out == "plots" else r["plots"][f * (rec + pad):][:rec],
                   None if leave_out == "labels" else r["labels"][f * 4 * MD:][:4 * MD])
    finally:
        for g in (d_in, out, plots, labels):
            g.release()
