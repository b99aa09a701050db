"""tests/_guard.py on a CPU box: a fake context whose sarx_malloc / sarx_free / sarx_memset / sarx_memcpy_* act on host memory
through ctypes, a correct fake kernel and three deliberately wrong ones written in NumPy.  This is where the suite shows that the
guard tests of tests/test_gpu_guard.py have teeth; no real kernel is ever broken for it.  Also: the case table of
test_gpu_guard.py names every device entry point the three signature tables bind."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _guard import GuardedBuffer, guarded, guarded_run, zone_bytes  # noqa: E402


class _FakeLib:
    """The five memory entry points of include/sarx.h on host memory."""

    def __init__(self):
        self.blocks = {}

    def sarx_malloc(self, h, nbytes, out):
        blk = (C.c_ubyte * max(int(nbytes), 1))()
        addr = C.addressof(blk)
        self.blocks[addr] = blk
        out._obj.value = addr                     # `out` is ctypes.byref(c_void_p)
        return 0

    def sarx_free(self, h, ptr):
        return 0 if self.blocks.pop(ptr, None) is not None else -1

    def sarx_memset(self, h, ptr, value, nbytes):
        C.memset(ptr, value, nbytes)
        return 0

    def sarx_memcpy_h2d(self, h, dst, src, nbytes):
        C.memmove(dst, src, nbytes)
        return 0

    sarx_memcpy_d2h = sarx_memcpy_h2d

    def sarx_last_error(self, h):
        return b"fake"


class _FakeCtx:
    def __init__(self):
        self.lib, self.h, self._live = _FakeLib(), 1, {}


def _mem(ptr, count, dtype):
    """NumPy view of `count` elements at a 'device' address (may start before or reach past a payload: what a kernel can do)."""
    dtype = np.dtype(dtype)
    return np.frombuffer((C.c_ubyte * (count * dtype.itemsize)).from_address(ptr), dtype=dtype)


@pytest.fixture
def ctx():
    return _FakeCtx()


N = 1000


def _case(ctx, kernel):
    x = np.random.default_rng(1).standard_normal(N).astype(np.float32)
    d_in, d_out = guarded(ctx, x), GuardedBuffer(ctx, N * 4)
    return guarded_run(lambda: kernel(d_in.ptr, d_out.ptr), {"x": (d_in, x)}, {"y": d_out}, dtypes={"y": np.float32})[0], x, d_out


def _double(p_in, p_out):
    _mem(p_out, N, np.float32)[:] = 2 * _mem(p_in, N, np.float32)


def test_layout_alignment_and_zone_condition(ctx):
    assert zone_bytes() == 65536 and zone_bytes(13200 * 8) == 212992 and zone_bytes(13200 * 8) >= 2 * 13200 * 8
    assert zone_bytes(16384 * 8) == 262144 and zone_bytes(33000) % 4096 == 0
    b = GuardedBuffer(ctx, 100)
    assert b.ptr - b.base == 65536 and b.nbytes == 100 and len(ctx.lib.blocks) == 1          # one allocation
    assert (_mem(b.base, 65536, np.uint8) == 0xFF).all() and (_mem(b.ptr + 100, 65536, np.uint8) == 0xFF).all()
    o = GuardedBuffer(ctx, 100, offset=8)
    assert o.ptr - o.base == 65536 + 8 and o.check_zones() == []
    for bad in (4096, 65536 + 512):
        with pytest.raises(ValueError):
            GuardedBuffer(ctx, 100, zone=bad)
    b.upload(np.arange(25, dtype=np.int32))
    np.testing.assert_array_equal(b.download(np.int32), np.arange(25))
    assert np.isnan(b.poison().download(np.float32)).all() and (b.download(np.int32) == -1).all()
    w = GuardedBuffer(ctx, 80)
    assert np.isnan(w.poison().download(np.float64)).all()
    assert not b.zero().download(np.uint8).any() and b.check_zones() == []
    with pytest.raises(ValueError):
        b.upload(np.zeros(101, np.uint8))
    for buf in (b, o, w):
        buf.release()
    assert not ctx.lib.blocks and not ctx._live


def test_correct_kernel_passes(ctx):
    findings, x, d_out = _case(ctx, _double)
    assert findings == []
    np.testing.assert_array_equal(d_out.download(np.float32), 2 * x)


def test_one_element_past_the_end_is_reported(ctx):
    def kernel(p_in, p_out):
        _mem(p_out, N + 1, np.float32)[:N + 1] = np.append(2 * _mem(p_in, N, np.float32), np.float32(1.0))
    findings, _, _ = _case(ctx, kernel)
    assert {f.kind for f in findings} == {"zone"} and len(findings) == 2           # once per run
    f = findings[0]
    assert (f.buffer, f.side, f.first, f.last, f.count) == ("y", "after", 4 * N, 4 * N + 3, 4)


def test_one_element_before_the_start_is_reported(ctx):
    def kernel(p_in, p_out):
        _double(p_in, p_out)
        _mem(p_out - 8, 1, np.complex64)[0] = 3 + 4j
    findings, _, _ = _case(ctx, kernel)
    assert {f.kind for f in findings} == {"zone"}
    f = findings[0]
    assert (f.buffer, f.side, f.first, f.last, f.count) == ("y", "before", -8, -1, 8)
    # ... with the payload at offset 8 the skipped bytes are canaries as well
    d = GuardedBuffer(ctx, 64, offset=8)
    _mem(d.ptr - 4, 1, np.int32)[0] = 7
    (dmg,) = d.check_zones()
    assert (dmg.side, dmg.first, dmg.last, dmg.count) == ("before", -4, -1, 4)
    d.restore_zones()
    assert d.check_zones() == []


def test_one_unwritten_element_is_reported(ctx):
    def kernel(p_in, p_out):
        y = 2 * _mem(p_in, N, np.float32)
        out = _mem(p_out, N, np.float32)
        out[:777] = y[:777]
        out[778:] = y[778:]
    findings, _, _ = _case(ctx, kernel)
    unwritten = [f for f in findings if f.kind == "unwritten"]
    assert len(unwritten) == 1 and (unwritten[0].first, unwritten[0].last, unwritten[0].count) == (777 * 4, 777 * 4 + 3, 4)
    nonfinite = [f for f in findings if f.kind == "nonfinite"]                       # the poison shows as a NaN in the result
    assert len(nonfinite) == 1 and nonfinite[0].run == "poisoned" and nonfinite[0].first == 777 * 4
    assert {f.kind for f in findings} == {"unwritten", "nonfinite"}


def test_accumulating_kernel_is_reported(ctx):
    def kernel(p_in, p_out):
        _mem(p_out, N, np.float32)[5] += 1.0                     # += instead of =
        out = _mem(p_out, N, np.float32)
        keep = out[5]
        _double(p_in, p_out)
        out[5] = keep
    findings, _, _ = _case(ctx, kernel)
    assert any(f.kind == "unwritten" and f.first // 4 == 5 == f.last // 4 for f in findings)


def test_modified_input_is_reported(ctx):
    def kernel(p_in, p_out):
        _double(p_in, p_out)
        _mem(p_in, N, np.float32)[123] = 0.0
    findings, _, _ = _case(ctx, kernel)
    assert {f.kind for f in findings} == {"input"} and len(findings) == 2
    f = findings[0]
    assert f.buffer == "x" and 123 * 4 <= f.first <= f.last <= 123 * 4 + 3


def test_out_of_bounds_read_shows_as_nan(ctx):
    """A read one element past the input, weighted into the last output: invisible in a parity test whose neighbour is zero."""
    def kernel(p_in, p_out):
        x = _mem(p_in, N + 1, np.float32)
        _mem(p_out, N, np.float32)[:] = 2 * x[:N] + 0 * x[1:]
    findings, _, _ = _case(ctx, kernel)
    assert {f.kind for f in findings} == {"nonfinite"}
    assert all((f.first, f.last) == (4 * (N - 1), 4 * N - 1) for f in findings)


def test_promised_prefix_and_bytes_left_alone(ctx):
    """An output of which the header promises a part (a report list up to its count): the rest must stay 0xFF."""
    d_out = GuardedBuffer(ctx, 64)

    def good():
        _mem(d_out.ptr, 4, np.int32)[:] = [3, 1, 2, 3]

    def bad():
        good()
        _mem(d_out.ptr, 16, np.int32)[9] = 0
    count = lambda p: 4 + 4 * int(p[:4].view(np.int32)[0])
    assert guarded_run(good, {}, {"list": d_out}, promised={"list": count})[0] == []
    findings = guarded_run(bad, {}, {"list": d_out}, promised={"list": count})[0]
    assert [(f.kind, f.first, f.last) for f in findings] == [("stray", 36, 39)]


def test_case_table_names_every_device_entry_point():
    """A new *_dev entry point cannot arrive without a bounds case: every such name of the three signature tables, sarx_csa_pass
    and the strided copies must be in the case table of test_gpu_guard.py or in its commented exclusion list."""
    from sarx import _ffi
    import test_gpu_guard as g
    names = [n for tab in (_ffi.SIGNATURES, _ffi.GMTI_SIGNATURES, _ffi.REFOCUS_SIGNATURES) for n in tab]
    need = {n for n in names if n.endswith("_dev") or n.endswith("_dev2")} | {"sarx_csa_pass", "sarx_memcpy2d_h2d",
                                                                               "sarx_memcpy2d_d2h", "sarx_fill_noise_c64"}
    assert len(need) >= 27
    covered = g.covered_entry_points()
    missing = sorted(need - covered - set(g.EXCLUDED))
    assert not missing, f"no guard case for {missing}"
    assert not set(g.EXCLUDED) & covered and all(len(why) > 10 for why in g.EXCLUDED.values())
    assert covered <= set(names), sorted(covered - set(names))
