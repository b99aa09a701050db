"""What the detection chain's device entry points refuse once they hold a live context (include/sarx_gmti.h, sarx_refocus.h,
sarx_track.h, sarx_balance.h): a missing buffer, a misaligned one, an empty image, a short or odd stride, a negative frame count.
The refusals before the context check run without a device (tests/test_gmti.py and its siblings); those of the OS-CFAR, the plot
extraction, the ATI gate and the coherence have tests of their own beside their kernels.  Each case here states the code and a
word of the message, nothing is launched - every buffer is still the 0xFF it was filled with - and a plain call afterwards runs."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2          # SARX_ERR_INVALID, SARX_ERR_UNSUPPORTED
N_AZ, N_RG, MD = 64, 16, 8             # the shortest refocus chip is 64 rows; eight reports
SLOT = 16 + 48 * MD
N_HYP = 3


class Rig:
    """The buffers of every entry point, the parameter blocks, and the tables of bad calls."""

    def __init__(self):
        import sarx
        from sarx import _ffi, balance, track
        self.ctx = ctx = sarx.default_context()
        self.lib = ctx.lib
        self.gmti = _ffi.GmtiParams(2, 2, 4, 4, 10.0, 8, MD)
        self.refocus = sarx.RefocusParams(chip=(64, 1), v_along=(-5.0, 5.0), n_hyp=N_HYP).c_params(0.03, 100.0, 1000.0, 5000.0, 1.0, 0.0)
        self.track = sarx.TrackParams(max_tracks=16, max_detections=MD).c_params()
        lo = _ffi.BALANCE_MIN_BLOCK
        self.balance = sarx.BalanceParams(block=(lo, lo)).c_params(N_AZ, N_RG)
        img = N_AZ * N_RG * 8
        sizes = dict(slc1=img, slc2=img, slc2_out=img, mag=img // 2, stack=2 * SLOT, records=48 * MD, curves=4 * MD * N_HYP, chips=8 * 64 * MD,
                     table=track.table_bytes(self.track), workspace=track.workspace_bytes(self.track), assoc=2 * 4 * MD,
                     bal_table=balance.table_bytes(self.balance, N_AZ, N_RG), bal_workspace=balance.workspace_bytes(self.balance, N_AZ, N_RG))
        self.bufs = {k: ctx.alloc(v) for k, v in sizes.items()}

    def release(self):
        for b in self.bufs.values():
            b.release()

    def fill(self, byte):
        from sarx._ffi import check
        for b in self.bufs.values():
            check(self.lib.sarx_memset(self.ctx.h, b.ptr, byte, b.nbytes), self.ctx.h)

    def touched(self):
        """The buffers that are no longer all 0xFF."""
        self.ctx.sync()
        return [k for k, b in self.bufs.items() if not (b.download(np.uint8, (b.nbytes,)) == 0xFF).all()]

    def last_error(self):
        return self.lib.sarx_last_error(self.ctx.h).decode()

    def entry(self, name):
        """(call, the good arguments by name): call(**changed) passes the good arguments with some replaced."""
        p = {k: b.ptr for k, b in self.bufs.items()}
        h, ref = self.ctx.h, C.byref
        good = {
            "sarx_gmti_cfar_dev": dict(mag=p["mag"], n_az=N_AZ, n_rg=N_RG, params=self.gmti, reports=p["stack"] + 16, header=p["stack"]),
            "sarx_gmti_refine_dev": dict(slc1=p["slc1"], slc2=p["slc2"], n_az=N_AZ, n_rg=N_RG, cal_phase=0.0, reports=p["stack"] + 16,
                                         header=p["stack"], max_det=MD),
            "sarx_refocus_dev": dict(slc1=p["slc1"], slc2=p["slc2"], n_az=N_AZ, n_rg=N_RG, params=self.refocus, reports=p["stack"] + 16,
                                     header=p["stack"], max_det=MD, records=p["records"], curves=p["curves"], chips=p["chips"]),
            "sarx_track_init_dev": dict(params=self.track, table=p["table"]),
            "sarx_track_step_dev": dict(params=self.track, slot=p["stack"], frame=0, table=p["table"], assoc=p["assoc"], workspace=p["workspace"]),
            "sarx_track_run_dev": dict(params=self.track, stack=p["stack"], stride=SLOT, n_frames=2, table=p["table"], assoc=p["assoc"],
                                       workspace=p["workspace"]),
            "sarx_balance_estimate_dev": dict(slc1=p["slc1"], slc2=p["slc2"], n_az=N_AZ, n_rg=N_RG, params=self.balance, table=p["bal_table"],
                                              workspace=p["bal_workspace"]),
            "sarx_balance_apply_dev": dict(slc1=p["slc1"], slc2=p["slc2"], n_az=N_AZ, n_rg=N_RG, params=self.balance, table=p["bal_table"],
                                           out=p["slc2_out"], dpca_mag=p["mag"]),
        }[name]

        def call(**changed):
            args = [ref(v) if isinstance(v, C.Structure) else v for v in {**good, **changed}.values()]
            return getattr(self.lib, name)(h, *args)

        return call, good


def edited(params, **fields):
    """A copy of a ctypes parameter block with some fields changed."""
    q = type(params).from_buffer_copy(params)
    for k, v in fields.items():
        setattr(q, k, v)
    return q


# entry point -> the buffers that must be there, every buffer with its alignment, and the refusals that are the entry point's own:
# (case, changed arguments, code, a word of the message as the library words it)
SIZES = [("n_az 0", dict(n_az=0), INVALID, "size"), ("n_rg 0", dict(n_rg=0), INVALID, "size"), ("n_az -1", dict(n_az=-1), INVALID, "size")]
TABLE = {
    "sarx_gmti_cfar_dev": (("mag", "reports", "header"), dict(reports=8, header=4), SIZES + [          # the plane's alignment is not checked
        ("max_detections 0", lambda r: dict(params=edited(r.gmti, max_detections=0)), INVALID, "max_detections"),
        ("guard + train 33", lambda r: dict(params=edited(r.gmti, train_az=31)), UNSUPPORTED, "exceed")]),
    "sarx_gmti_refine_dev": (("slc1", "slc2", "reports", "header"), dict(reports=8, header=4), SIZES + [
        ("max_det 0", dict(max_det=0), INVALID, "max_detections"), ("cal_phase nan", dict(cal_phase=math.nan), INVALID, "cal_phase")]),
    "sarx_refocus_dev": (("slc1", "reports", "header", "records"),
                         dict(slc1=8, slc2=8, reports=8, header=4, records=8, curves=4, chips=8), SIZES + [
        ("DPCA without slc2", dict(slc2=None), INVALID, "slc2"), ("max_det 0", dict(max_det=0), INVALID, "max_detections"),
        ("chip longer than the image", lambda r: dict(params=edited(r.refocus, chip_az=128)), INVALID, "exceeds")]),
    "sarx_track_init_dev": (("table",), dict(table=8), []),
    "sarx_track_step_dev": (("slot", "table", "workspace"), dict(slot=8, table=8, workspace=8, assoc=4), [
        ("frame -1", dict(frame=-1), INVALID, "frame_index")]),
    "sarx_track_run_dev": (("stack", "table", "workspace"), dict(stack=8, table=8, workspace=8, assoc=4), [
        ("stride 8 short", dict(stride=SLOT - 8), INVALID, "stride"), ("stride not a multiple of 8", dict(stride=SLOT + 4), INVALID, "stride"),
        ("n_frames -1", dict(n_frames=-1), INVALID, "n_frames")]),
    "sarx_balance_estimate_dev": (("slc1", "slc2", "table", "workspace"), dict(slc1=8, slc2=8, table=8, workspace=8), SIZES),
    "sarx_balance_apply_dev": (("slc2", "table", "out"), dict(slc1=8, slc2=8, table=8, out=8, dpca_mag=4), SIZES + [
        ("dpca_mag without slc1", dict(slc1=None), INVALID, "slc1")]),
}
# what runs before an entry point's plain call so that it reads what it expects (buffers zeroed: no report, no track)
BEFORE = {"sarx_track_step_dev": ["sarx_track_init_dev"], "sarx_track_run_dev": ["sarx_track_init_dev"],
          "sarx_balance_apply_dev": ["sarx_balance_estimate_dev"]}


def bad_calls(rig, name):
    """[(case, changed arguments, code, word)] of one entry point: each required pointer NULL, each pointer off its alignment by
    half of it (8-byte buffers by 4, 4-byte buffers by 2), then its own."""
    required, aligned, own = TABLE[name]
    _, good = rig.entry(name)
    cases = [(f"{k} NULL", {k: None}, INVALID, "NULL") for k in required]
    cases += [(f"{k} + {a // 2}", {k: good[k] + a // 2}, INVALID, "misaligned") for k, a in aligned.items()]
    return cases + [(case, ch(rig) if callable(ch) else ch, rc, word) for case, ch, rc, word in own]


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.release()


@pytest.mark.parametrize("name", list(TABLE))
def test_arguments_the_header_forbids(rig, name):
    call, _ = rig.entry(name)
    rig.fill(0xFF)
    for case, changed, rc, word in bad_calls(rig, name):
        got = call(**changed)
        print(f"{name} / {case} / {got} / {rig.last_error()}")
        assert got == rc and word in rig.last_error(), (case, got, rig.last_error())
    assert rig.touched() == []
    rig.fill(0)
    for first in BEFORE.get(name, []):
        assert rig.entry(first)[0]() == 0, rig.last_error()
    assert call() == 0, rig.last_error()                     # and the plain call still goes
    rig.ctx.sync()
