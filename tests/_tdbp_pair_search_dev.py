"""What tests/test_gpu_tdbp_pair_search.py and tests/test_gpu_tdbp_pair_search_guard.py share to call sarx_tdbp_pair_search_dev and
_host directly (ctypes, caller-held buffers): the slot of a list of (i, j), the argument list, and the byte masks of what the
header promises to write.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

REC_BYTES, BEST_BYTES = 32, 80


def slot_of(positions, max_detections, count=None, overflow=0):
    """A slot's bytes: header (count = len(positions) unless given, overflow) and the reports carrying (i, j) alone."""
    from sarx import slot
    rep = np.zeros(len(positions), slot.REPORT_DTYPE)
    if len(positions):
        rep["i"], rep["j"] = np.asarray(positions)[:, 0], np.asarray(positions)[:, 1]
    raw = np.zeros(slot.slot_bytes(max_detections), np.uint8)
    raw[:8].view("<u4")[:] = (len(positions) if count is None else count, overflow)
    raw[slot.HEADER_BYTES:slot.HEADER_BYTES + rep.nbytes] = rep.view(np.uint8)
    return raw


def call(lib, entry, plan, sc, scene_size, shift, hyps, raw0, raw1, slot_ptr, max_detections, chip, source, rec, best, chips):
    """One call of sarx_tdbp_pair_search_dev / _host (entry) on a scene dict of tests/_tdbp_pair_numpy.py; pointers as integers."""
    from sarx.tdbp_pair import pair_params
    from sarx.tdbp_pair_search import search_params
    n_p = len(sc["t_vec"])
    pos, vel, tp = (np.ascontiguousarray(sc[n], dtype=np.float64) for n in ("pos", "vel", "t_vec"))
    hyp = np.ascontiguousarray(hyps, dtype=np.float64)
    prm = pair_params(n_p, sc["rx_offsets"], sc["chirp_centre"], shift)
    sp = search_params(chip, len(hyp), source)
    return getattr(lib, entry)(plan.h, raw0, raw1, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(sc["t_start"]), float(scene_size),
                               C.byref(prm), hyp.ctypes.data, slot_ptr + 16, slot_ptr, int(max_detections), C.byref(sp), rec, best, chips)


def promised(positions, nx, ny, max_detections, n_hyp, chip, count=None):
    """Byte masks {"rec", "best", "chips"} over the whole output arrays of what a usable slot makes the library write: everything
    of a report inside the grid, the first four bytes (k_best) of the best record of one outside it, nothing past the count."""
    chip_bytes = 2 * chip[0] * chip[1] * 16
    m = {"rec": np.zeros((max_detections, n_hyp * REC_BYTES), bool), "best": np.zeros((max_detections, BEST_BYTES), bool),
         "chips": np.zeros((max_detections, n_hyp * chip_bytes), bool)}
    for r, (i, j) in enumerate(positions[:len(positions) if count is None else count]):
        if 0 <= i < ny and 0 <= j < nx:
            for a in m.values():
                a[r] = True
        else:
            m["best"][r, :4] = True
    return {k: v.reshape(-1) for k, v in m.items()}
