"""Guard bands and poison around the two device entry points of include/sarx_pga.h (tests/_guard.py, the protocol of
tests/test_gpu_guard.py): every device argument is a GuardedBuffer, each case runs once with every output poisoned (0xFF) and once
zeroed.  The promised bytes - the n_rg columns of every frame of d_out, phi_tot, the n_iter + 1 records of every frame - must be
bit-identical and finite; the pad columns n_rg .. ld - 1 of d_out, the elements between two frames and the records beyond
n_iter keep their poison; every zone stays clean and d_in is unchanged.  The workspace's content is not defined by the header: only
its extent is watched."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pga_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

# (L, n_rg, pad columns, frames, elements between a frame's end and the next one's start)
LAYOUTS = [(64, 1, 0, 1, 0), (64, 1, 3, 2, 5), (128, 17, 5, 3, 37), (256, 33, 0, 2, 0), (512, 20, 1, 1, 0), (1024, 9, 3, 1, 0)]
CASES = [(g, off) for g in LAYOUTS for off in (0, 8)]
N_ITER, SPARE_RECORDS = 2, 3


def _id(c):
    (n_az, n_rg, pad, nf, gap), off = c
    return f"{n_az}x{n_rg}-ld{n_rg + pad}-f{nf}-off{off}"


def _stack(n_az, n_rg, pad, nf, gap):
    """(host buffer with NaN wherever no frame element lies, frames, ld, stride, byte mask of the frames' elements)"""
    ld = n_rg + pad
    stride = n_az * ld + gap
    n = (nf - 1) * stride + (n_az - 1) * ld + n_rg
    host = np.full(n, np.nan + 1j * np.nan, np.complex64)
    mask = np.zeros(n, bool)
    frames = []
    for f in range(nf):
        img = ref.apply(ref.scene(n_az, n_rg, min(4, n_rg), 20 + f), (0.5 + 0.25 * f) * ref.error("cubic_sine", n_az), +1).astype(np.complex64)
        idx = f * stride + np.arange(n_az)[:, None] * ld + np.arange(n_rg)[None, :]
        host[idx] = img
        mask[idx] = True
        frames.append(img)
    return host, frames, ld, stride, np.repeat(mask, 8)


@pytest.mark.parametrize("layout,off", CASES, ids=[_id(c) for c in CASES])
def test_pga_guard(layout, off):
    import sarx
    K = importlib.import_module("sarx.pga")
    ctx = sarx.default_context()
    n_az, n_rg, pad, nf, gap = layout
    host, frames, ld, stride, elems = _stack(*layout)
    hw = ref.default_half_widths(n_az, N_ITER)
    cp = sarx.PgaParams(n_iter=N_ITER, half_widths=hw).c_params(n_az)
    z = zone_bytes(ld * 8)
    d_in = guarded(ctx, host, z, offset=off)
    n_rec = nf * (N_ITER + 1)
    outs = {"out": GuardedBuffer(ctx, host.nbytes, z, offset=off), "phase": GuardedBuffer(ctx, nf * n_az * 8, offset=off),
            "records": GuardedBuffer(ctx, (n_rec + SPARE_RECORDS) * 32, offset=off),
            "workspace": GuardedBuffer(ctx, K.workspace_bytes(cp, n_az, n_rg, ld, nf, stride), offset=off)}
    try:
        findings, res = guarded_run(lambda: K.enqueue(ctx, d_in.ptr, outs["out"].ptr, n_az, n_rg, ld, nf, stride, cp, outs["phase"].ptr,
                                                      outs["records"].ptr, outs["workspace"].ptr),
                                    {"in": (d_in, host)}, outs, promised={"out": elems, "records": n_rec * 32, "workspace": None},
                                    dtypes={"out": np.float32, "phase": np.float64}, sync=ctx.sync)
        assert not findings, findings
        out = res["poisoned"]["out"].view(np.complex64)
        rec = res["poisoned"]["records"][:n_rec * 32].view(K.RECORD_DTYPE).reshape(nf, N_ITER + 1)
        ph = res["poisoned"]["phase"].view(np.float64).reshape(nf, n_az)
        for f, img in enumerate(frames):
            got = out[f * stride + np.arange(n_az)[:, None] * ld + np.arange(n_rg)[None, :]]
            want = ref.apply(img, ph[f], -1)                               # the output is the input under the phase the call returned
            assert np.linalg.norm(got - want) <= 1e-4 * np.linalg.norm(want)
            assert np.isfinite(rec[f]["s2"]).all() and np.isfinite(rec[f]["s4"]).all() and np.isfinite(rec[f]["rms_phase"]).all()
            assert (rec[f]["n_cols_used"] == n_rg).all() and (rec[f]["n_bins_supported"] == n_az).all()      # min_contrast 0, floor 0
    finally:
        for g in [d_in] + list(outs.values()):
            g.release()


@pytest.mark.parametrize("layout,off", CASES, ids=[_id(c) for c in CASES])
def test_apply_guard(layout, off):
    import sarx
    K = importlib.import_module("sarx.pga")
    ctx = sarx.default_context()
    n_az, n_rg, pad, nf, gap = layout
    host, frames, ld, stride, elems = _stack(*layout)
    phase = np.stack([(1.0 + f) * ref.error("quadratic", n_az) for f in range(nf)])
    z = zone_bytes(ld * 8)
    d_in, d_ph = guarded(ctx, host, z, offset=off), guarded(ctx, phase, offset=off)
    outs = {"out": GuardedBuffer(ctx, host.nbytes, z, offset=off)}
    try:
        for ph_stride in (n_az, 0):
            findings, res = guarded_run(lambda: K.enqueue_apply(ctx, d_in.ptr, outs["out"].ptr, n_az, n_rg, ld, nf, stride, d_ph.ptr, ph_stride, 1),
                                        {"in": (d_in, host), "phase": (d_ph, phase)}, outs, promised={"out": elems},
                                        dtypes={"out": np.float32}, sync=ctx.sync)
            assert not findings, (ph_stride, findings)
            out = res["poisoned"]["out"].view(np.complex64)
            for f, img in enumerate(frames):
                want = ref.apply(img, phase[f if ph_stride else 0], +1)
                got = out[f * stride + np.arange(n_az)[:, None] * ld + np.arange(n_rg)[None, :]]
                assert np.linalg.norm(got - want) <= 1e-4 * np.linalg.norm(want)
    finally:
        for g in [d_in, d_ph] + list(outs.values()):
            g.release()
