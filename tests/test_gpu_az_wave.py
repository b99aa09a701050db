"""The wave-private azimuth tiles (az_wave.hip, SARX_AZ_IMPL=1, the default) against az_tile_kernel (SARX_AZ_IMPL=0) at
16384^2 on the same device input: each of the four 128-point steps of the four-step transform (sarx_csa_pass ids 110-113)
and a whole focus.  The transforms add in another order, so the images agree to rounding, not bit for bit.

Role: the full-size cross-check of the two routes (two workgroups and more per tile row, 2 GiB images, the whole focus).  Neither
side is a reference here; what each launch must produce is stated by tests/test_gpu_az_steps.py, which holds both routes - and every
other four-step size, width and epilogue - by the complex128 step oracle on images a few columns wide, in seconds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 16384
TOL = 1e-6


@pytest.fixture(scope="module")
def sx():
    import sarx
    return sarx


@pytest.fixture(scope="module")
def ctx(sx):
    return sx.default_context()


@pytest.fixture(scope="module")
def plans(sx, ctx):
    import os
    from sarx import _ffi, radar
    args = radar.focus_args(N)
    out = {}
    for impl in ("0", "1"):
        saved = os.environ.get("SARX_AZ_IMPL")
        os.environ["SARX_AZ_IMPL"] = impl
        try:
            out[impl] = sx.CsaPlan(ctx, N, N, *args, flags=_ffi.FUSE_RANGE)
        finally:
            if saved is None:
                os.environ.pop("SARX_AZ_IMPL")
            else:
                os.environ["SARX_AZ_IMPL"] = saved
    yield out
    for p in out.values():
        p.close()


def _rel_l2(ctx, a, b, block=1024):
    """||a - b|| / ||b|| over two whole N x N device images, downloaded in row blocks"""
    from sarx.engine import download_block
    num = den = 0.0
    for r0 in range(0, N, block):
        x = download_block(ctx, a.ptr, N, r0, block, 0, N).astype(np.complex128)
        y = download_block(ctx, b.ptr, N, r0, block, 0, N).astype(np.complex128)
        num += float(np.sum(np.abs(x - y) ** 2))
        den += float(np.sum(np.abs(y) ** 2))
    assert den > 0
    return np.sqrt(num / den)


@pytest.mark.parametrize("pass_id", [110, 111, 112, 113], ids=["fwd_A_twiddle", "fwd_B_phi1", "inv_A_twiddle", "inv_B_scale_max"])
def test_each_step_against_the_tile_kernel(sx, ctx, plans, pass_id):
    from sarx import _ffi
    px = N * N
    x, y_old, y_new = ctx.alloc(px * 8), ctx.alloc(px * 8), ctx.alloc(px * 8)
    m_old, m_new = ctx.alloc(_ffi.MAX_SLOT_BYTES), ctx.alloc(_ffi.MAX_SLOT_BYTES)
    try:
        ctx.fill_noise(x, px, 1000 + pass_id)
        plans["0"].set_max_slot(m_old)
        plans["1"].set_max_slot(m_new)
        plans["0"].run_pass(pass_id, x, y_old)
        plans["1"].run_pass(pass_id, x, y_new)
        ctx.sync()
        err = _rel_l2(ctx, y_new, y_old)
        assert err < TOL, err
        if pass_id == 113:
            mo = m_old.download(np.float32, (_ffi.MAX_SLOT_BYTES // 4,))[::32].max()
            mn = m_new.download(np.float32, (_ffi.MAX_SLOT_BYTES // 4,))[::32].max()
            assert mo > 0 and abs(mn - mo) <= TOL * mo, (mn, mo)
    finally:
        plans["0"].set_max_slot(None)
        plans["1"].set_max_slot(None)
        for b in (x, y_old, y_new, m_old, m_new):
            b.release()


def test_whole_focus_against_the_tile_kernel(sx, ctx, plans):
    px = N * N
    x, img_old, img_new = ctx.alloc(px * 8), ctx.alloc(px * 8), ctx.alloc(px * 8)
    try:
        ctx.fill_noise(x, px, 20261016)
        plans["0"].focus_dev(x, img_old)
        plans["1"].focus_dev(x, img_new)
        ctx.sync()
        err = _rel_l2(ctx, img_new, img_old)
        assert err < TOL, err
    finally:
        for b in (x, img_old, img_new):
            b.release()
