"""Guard bands and poison around the two device entry points of include/sarx_balance.h (tests/_guard.py, the protocol of
tests/test_gpu_guard.py): every device argument is a GuardedBuffer, each case runs once with every output poisoned (0xFF) and once
zeroed; the promised bytes - the whole table, slc2_out, dpca_mag - must be bit-identical and finite, every zone clean and every
const input unchanged.  The workspace's content is not defined by the header (scratch): only its extent is watched.  Results are
also held against the restatement at test_gpu_balance.py's bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _balance_numpy as ref  # noqa: E402
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL = 1e-4


def _rand(shape, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(np.complex64)


# (id, shape, block, payload offsets in bytes: images and table / dpca_mag, in place)
CASES = [("96x80", (96, 80), (32, 16), 0, 0, False),
         ("1000x777-offset0", (1000, 777), (256, 64), 0, 0, False),
         ("1000x777-offset4", (1000, 777), (256, 64), 0, 4, False),          # the fp32 plane 4 bytes off: no 8-byte stores into it
         ("1000x777-offset8", (1000, 777), (256, 64), 8, 8, False),          # everything 8 bytes past a 16-byte boundary
         ("96x80-offset8", (96, 80), (32, 16), 8, 8, False),                 # even rows, views 8 bytes off: the 8-byte loads
         ("96x80-in-place", (96, 80), (32, 16), 0, 0, True),
         ("1000x777-in-place-offset8", (1000, 777), (256, 64), 8, 4, True)]


@pytest.mark.parametrize("cid,shape,block,off,off_dm,in_place", CASES, ids=[c[0] for c in CASES])
def test_guard(cid, shape, block, off, off_dm, in_place):
    import sarx
    from sarx import balance as B
    ctx = sarx.default_context()
    n_az, n_rg = shape
    a = _rand(shape, n_az + n_rg)
    b = (a * (0.7 - 0.4j) + 0.3 * _rand(shape, n_az + n_rg + 1)).astype(np.complex64)
    p = sarx.BalanceParams(block=block, min_count=1)
    cp = p.c_params(n_az, n_rg, 9.0)
    z = zone_bytes(n_rg * 8)
    d1 = guarded(ctx, a, z, offset=off)
    d2 = guarded(ctx, b, z, offset=off)
    table = GuardedBuffer(ctx, B.table_bytes(cp, n_az, n_rg), offset=off)
    ws = GuardedBuffer(ctx, B.workspace_bytes(cp, n_az, n_rg))
    dm = GuardedBuffer(ctx, n_az * n_rg * 4, z, offset=off_dm)
    out = d2 if in_place else GuardedBuffer(ctx, b.nbytes, z, offset=off)
    bufs = [d1, d2, table, ws, dm] + ([] if in_place else [out])
    t = ref.balance(a, b, block, "ls", "bilinear", 9.0, min_count=1)
    try:
        # estimate: the whole table is promised, the workspace is scratch
        findings, res = guarded_run(lambda: B.enqueue_estimate(ctx, d1.ptr, d2.ptr, n_az, n_rg, cp, table.ptr, ws.ptr),
                                    {"slc1": (d1, a), "slc2": (d2, b)}, {"table": table, "workspace": ws},
                                    promised={"workspace": None}, sync=ctx.sync)
        assert not findings, findings
        raw = res["poisoned"]["table"]
        cb = B.ChannelBalance(raw, shape, block, "bilinear", 9.0)
        hdr = raw[:64].view(B.HEADER_DTYPE)[0]
        rec = raw[64:].view(B.RECORD_DTYPE)
        assert hdr["reserved"] == 0 and (rec["reserved"] == 0).all()
        for k in ("w_re", "w_im", "coherence", "s11", "s22"):
            assert np.isfinite(hdr[k])
        for k in ("s12_re", "s12_im", "s11", "s22", "w_re", "w_im", "coherence"):
            assert np.isfinite(rec[k]).all(), k
        np.testing.assert_array_equal(cb.counts, t["n"])
        np.testing.assert_array_equal(cb.valid, t["valid"])
        np.testing.assert_allclose(cb.s11, t["s11"], rtol=1e-12)
        np.testing.assert_allclose(cb.weights, t["w"], rtol=1e-11)

        # apply: slc2_out and dpca_mag are promised; the table is a const input now
        if in_place:
            # slc2 is input and output at once: the call uploads it afresh (after guarded_run has poisoned / zeroed the payload), so
            # the promise checked on it is the zones' and the two runs' agreement; dpca_mag keeps the full protocol
            def call():
                d2.upload(b)
                B.enqueue_apply(ctx, d1.ptr, d2.ptr, n_az, n_rg, cp, table.ptr, d2.ptr, dm.ptr)
            findings, res = guarded_run(call, {"slc1": (d1, a), "table": (table, raw)}, {"slc2": d2, "dpca_mag": dm},
                                        dtypes={"slc2": F32, "dpca_mag": F32}, sync=ctx.sync)
            assert not findings, findings
            got = [(res["poisoned"]["slc2"], res["poisoned"]["dpca_mag"])]
            img, plane = got[0][0].view(np.complex64).reshape(shape), got[0][1].view(F32).reshape(shape)
            d2.upload(b)                                               # and the out-of-place form gives the same bits
            tmp = GuardedBuffer(ctx, b.nbytes, z, offset=off)
            bufs.append(tmp)
            B.enqueue_apply(ctx, None, d2.ptr, n_az, n_rg, cp, table.ptr, tmp.ptr, None)
            ctx.sync()
            assert tmp.check_zones() == [] and np.array_equal(tmp.download(), got[0][0])
        else:
            findings, res = guarded_run(lambda: B.enqueue_apply(ctx, d1.ptr, d2.ptr, n_az, n_rg, cp, table.ptr, out.ptr, dm.ptr),
                                        {"slc1": (d1, a), "slc2": (d2, b), "table": (table, raw)}, {"slc2_out": out, "dpca_mag": dm},
                                        dtypes={"slc2_out": F32, "dpca_mag": F32}, sync=ctx.sync)
            assert not findings, findings
            img = res["poisoned"]["slc2_out"].view(np.complex64).reshape(shape)
            plane = res["poisoned"]["dpca_mag"].view(F32).reshape(shape)
            # without dpca_mag (slc1 = NULL) the image is the same and the plane is left alone
            dm.poison()
            out.poison()
            B.enqueue_apply(ctx, None, d2.ptr, n_az, n_rg, cp, table.ptr, out.ptr, None)
            ctx.sync()
            assert out.check_zones() == [] and (dm.download() == 0xFF).all()
            assert np.array_equal(out.download(), res["poisoned"]["slc2_out"])
        assert np.isfinite(img.view(F32)).all() and np.isfinite(plane).all()
        e_img = np.linalg.norm(img - t["slc2"]) / np.linalg.norm(t["slc2"])
        e_dm = np.linalg.norm(plane - t["dpca_mag"]) / np.linalg.norm(t["dpca_mag"])
        print(f"{cid}: slc2 rel-L2 {e_img:.2e}, dpca_mag rel-L2 {e_dm:.2e}")
        assert e_img < TOL and e_dm < TOL
    finally:
        for g in bufs:
            g.release()
