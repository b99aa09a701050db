"""fp64 NumPy restatement of the GMTI tracker (include/sarx_track.h states the semantics; csrc/track.hip implements them) - the
checker of tests/test_track.py and tests/test_gpu_track.py - and the seeded synthetic scenario both use.  No sarx import.

Every fp64 value is formed by the operations the header lists, one rounding each (NumPy fuses nothing), so the restatement and the
kernels make the same decisions and, on finite inputs, the same bits."""
import numpy as np

REPORT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("power", "<f8"), ("mean", "<f8"), ("interf_re", "<f8"), ("interf_im", "<f8"),
                         ("mag1", "<f4"), ("mag2", "<f4")])
HEADER_DTYPE = np.dtype([("n_live", "<u4"), ("n_confirmed", "<u4"), ("next_id", "<i4"), ("frames_done", "<u4"), ("births_total", "<u4"),
                         ("drops_total", "<u4"), ("error", "<u4"), ("error_frame", "<i4"), ("max_tracks", "<u4"), ("reserved", "<u4", (7,))])
SLOT_DTYPE = np.dtype([("p_i", "<f8"), ("p_j", "<f8"), ("v_i", "<f8"), ("v_j", "<f8"), ("sum_re", "<f8"), ("sum_im", "<f8"),
                       ("sum_power", "<f8"), ("max_ratio", "<f8"), ("id", "<i4"), ("status", "<u4"), ("hits", "<u4"), ("misses", "<u4"),
                       ("age", "<u4"), ("hist", "<u4"), ("last_frame", "<i4"), ("last_report", "<i4")])
assert REPORT_DTYPE.itemsize == 48 and HEADER_DTYPE.itemsize == 64 and SLOT_DTYPE.itemsize == 96
FREE, TENTATIVE, CONFIRMED = 0, 1, 2
OK, SLOT_OVERFLOW, TABLE_OVERFLOW = 0, 1, 2

DEFAULTS = dict(gate_az=4.0, gate_rg=4.0, alpha=0.5, beta=0.25, confirm_hits=3, confirm_window=5, max_misses=3, birth_ratio=0.0,
                max_tracks=1024, max_detections=4096)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def slot_bytes(reports, max_detections, count=None, overflow=0):
    """A GMTI slot as bytes: header (count, overflow, 0, 0), the reports, zeros up to max_detections reports."""
    reports = np.asarray(reports, REPORT_DTYPE)
    raw = np.zeros(16 + 48 * max_detections, np.uint8)
    raw[:8].view("<u4")[:] = (len(reports) if count is None else count, overflow)
    k = min(len(reports), max_detections)
    raw[16:16 + 48 * k] = reports[:k].view(np.uint8)
    return raw


def _popcount(x):
    return bin(int(x)).count("1")


class Tracker:
    """The table as a header record and a SLOT_DTYPE array; step() is one frame."""

    def __init__(self, p):
        self.p = p
        self.hdr = np.zeros((), HEADER_DTYPE)
        self.hdr["error_frame"] = -1
        self.hdr["max_tracks"] = p["max_tracks"]
        self.slots = np.zeros(p["max_tracks"], SLOT_DTYPE)
        self.assoc = []

    def table_bytes(self):
        return np.concatenate([np.frombuffer(self.hdr.tobytes(), np.uint8), self.slots.view(np.uint8)])

    def step(self, reports, frame, count=None, overflow=0):
        p, h, s = self.p, self.hdr, self.slots
        reports = np.asarray(reports, REPORT_DTYPE)
        n = len(reports) if count is None else int(count)
        row = np.full(p["max_detections"], -1, np.int32)
        self.assoc.append(row)
        if h["error"] != OK:
            return row
        if overflow or n > p["max_detections"]:
            h["error"], h["error_frame"] = SLOT_OVERFLOW, frame
            return row
        live = np.flatnonzero(s["status"] != FREE)
        zi, zj = reports["i"].astype(np.float64), reports["j"].astype(np.float64)
        ph_i, ph_j = s["p_i"][live] + s["v_i"][live], s["p_j"][live] + s["v_j"][live]
        best_t = np.full(n, -1)
        best_r = np.full(len(live), -1)
        if len(live) and n:
            a = (zi[None, :] - ph_i[:, None]) / p["gate_az"]
            b = (zj[None, :] - ph_j[:, None]) / p["gate_rg"]
            d2 = a * a + b * b
            d2 = np.where(d2 <= 1.0, d2, np.inf)
            br = np.argmin(d2, axis=1)                       # the first minimum: ties to the smaller r
            best_r = np.where(np.isfinite(d2[np.arange(len(live)), br]), br, -1)
            bt = np.argmin(d2, axis=0)                       # rows are in rising slot index: ties to the smaller slot
            best_t = np.where(np.isfinite(d2[bt, np.arange(n)]), bt, -1)     # an index into `live`
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = reports["power"] / reports["mean"]
        births = [r for r in range(n) if best_t[r] < 0 and (p["birth_ratio"] == 0.0 or ratio[r] >= p["birth_ratio"])]
        win = (1 << p["confirm_window"]) - 1
        drops = 0
        for k, t in enumerate(live):
            r = int(best_r[k])
            matched = r >= 0 and best_t[r] == k
            x = s[t]
            if matched:
                z = reports[r]
                ei, ej = zi[r] - ph_i[k], zj[r] - ph_j[k]
                x["p_i"], x["p_j"] = ph_i[k] + p["alpha"] * ei, ph_j[k] + p["alpha"] * ej
                x["v_i"], x["v_j"] = x["v_i"] + p["beta"] * ei, x["v_j"] + p["beta"] * ej
                x["hits"] += 1
                x["misses"], x["last_frame"], x["last_report"] = 0, frame, r
                x["sum_re"] += z["interf_re"]
                x["sum_im"] += z["interf_im"]
                x["sum_power"] += z["power"]
                if ratio[r] > x["max_ratio"]:
                    x["max_ratio"] = ratio[r]
                row[r] = x["id"]
            else:
                x["p_i"], x["p_j"] = ph_i[k], ph_j[k]
                x["misses"] += 1
            x["age"] += 1
            x["hist"] = ((int(x["hist"]) << 1) | int(matched)) & 0xFFFFFFFF
            if x["status"] == TENTATIVE and _popcount(int(x["hist"]) & win) >= p["confirm_hits"]:
                x["status"] = CONFIRMED
            if x["misses"] > p["max_misses"] or (x["status"] == TENTATIVE and x["age"] >= p["confirm_window"]):
                s[t] = np.zeros((), SLOT_DTYPE)
                drops += 1
        free = np.flatnonzero(s["status"] == FREE)
        made = 0
        if len(births) > len(free):
            h["error"], h["error_frame"] = TABLE_OVERFLOW, frame
        else:
            for k, r in enumerate(births):
                x = s[free[k]]
                z = reports[r]
                x["p_i"], x["p_j"] = zi[r], zj[r]
                x["sum_re"], x["sum_im"], x["sum_power"], x["max_ratio"] = z["interf_re"], z["interf_im"], z["power"], ratio[r]
                x["id"], x["status"], x["hits"], x["age"], x["hist"] = h["next_id"] + k, TENTATIVE, 1, 1, 1
                x["last_frame"], x["last_report"] = frame, r
                row[r] = x["id"]
            made = len(births)
            h["frames_done"] += 1
        h["n_live"] = np.count_nonzero(s["status"] != FREE)
        h["n_confirmed"] = np.count_nonzero(s["status"] == CONFIRMED)
        h["next_id"] += made
        h["births_total"] += made
        h["drops_total"] += drops
        return row


def run(frames, p):
    """frames: a list of report arrays, or of (reports, count, overflow).  Returns the Tracker after all steps."""
    tr = Tracker(p)
    for f, fr in enumerate(frames):
        if isinstance(fr, tuple):
            tr.step(fr[0], f, fr[1], fr[2])
        else:
            tr.step(fr, f)
    return tr


def unwrap(v_ati, range_rate, v_amb):
    """The ATI branch the coarse range rate picks: v_ati + 2 v_amb round((range_rate - v_ati) / (2 v_amb))."""
    return v_ati + 2.0 * v_amb * np.round((range_rate - v_ati) / (2.0 * v_amb))


# ---- the seeded scenario --------------------------------------------------------------------------------------------------------
def make_reports(ij, rng=None, v_phase=None):
    """Reports at integer pixels ij [k x 2], sorted by (i, j), duplicates dropped; power / mean = 20 .. 40, interferogram of unit
    magnitude times the power with phase v_phase (or seeded)."""
    ij = np.unique(np.asarray(ij, np.int64).reshape(-1, 2), axis=0)
    rep = np.zeros(len(ij), REPORT_DTYPE)
    rep["i"], rep["j"] = ij[:, 0], ij[:, 1]
    u = rng.random(len(ij)) if rng is not None else np.full(len(ij), 0.5)
    rep["mean"] = 1.0
    rep["power"] = 20.0 + 20.0 * u
    ph = (rng.uniform(-3, 3, len(ij)) if rng is not None else np.zeros(len(ij))) if v_phase is None else v_phase
    rep["interf_re"], rep["interf_im"] = rep["power"] * np.cos(ph), rep["power"] * np.sin(ph)
    rep["mag1"] = rep["mag2"] = np.sqrt(rep["power"])
    return rep


def scenario(seed=11, n_frames=24, n_targets=12, size=512, p_detect=0.9, n_false=6, speed=1.5):
    """Straight-line targets (two pairs of them crossing at mid-run), measured at the rounded pixel with probability p_detect,
    plus n_false uniform false alarms per frame.  Returns (frames, truth): frames[f] = report array, truth = dict with pos0,
    vel [n_targets x 2] and det[f][k] = the report index of target k in frame f or -1."""
    rng = np.random.default_rng(seed)
    pos0 = rng.uniform(0.2 * size, 0.8 * size, (n_targets, 2))
    ang = rng.uniform(0, 2 * np.pi, n_targets)
    vel = speed * rng.uniform(0.3, 1.0, n_targets)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    mid = (n_frames - 1) / 2.0
    for a, b in ((0, 1), (2, 3)):                                # crossing pairs: b passes through a's mid-run point at mid-run
        vel[b] = np.array([-vel[a][1], vel[a][0]]) * 1.3
        pos0[b] = pos0[a] + vel[a] * mid - vel[b] * mid
    frames, det = [], []
    for f in range(n_frames):
        z = np.rint(pos0 + vel * f).astype(np.int64)
        seen = rng.random(n_targets) < p_detect
        fa = rng.integers(0, size, (n_false, 2))
        ij = np.concatenate([z[seen], fa])
        rep = make_reports(ij, rng)
        key = {(int(a), int(b)): r for r, (a, b) in enumerate(zip(rep["i"], rep["j"]))}
        det.append(np.array([key[(int(z[k][0]), int(z[k][1]))] if seen[k] else -1 for k in range(n_targets)]))
        frames.append(rep)
    return frames, dict(pos0=pos0, vel=vel, det=det)


def score(tracker, frames, truth, p):
    """Per target: the ids its detections carried, the share of its detections under its main id; false-only confirmed tracks;
    the velocity error of the live tracks that end on a target."""
    assoc = tracker.assoc
    n_t = len(truth["pos0"])
    ids = [[int(assoc[f][truth["det"][f][k]]) for f in range(len(frames)) if truth["det"][f][k] >= 0] for k in range(n_t)]
    share, main = [], []
    for k in range(n_t):
        got = [x for x in ids[k] if x >= 0]
        vals, cnt = np.unique(got, return_counts=True) if got else (np.array([-1]), np.array([0]))
        main.append(int(vals[np.argmax(cnt)]))
        share.append(cnt.max() / max(len(ids[k]), 1))
    target_reports = [{int(truth["det"][f][k]) for k in range(n_t) if truth["det"][f][k] >= 0} for f in range(len(frames))]
    touched = set()                                              # ids that ever took a target's report
    for f in range(len(frames)):
        for r in target_reports[f]:
            if assoc[f][r] >= 0:
                touched.add(int(assoc[f][r]))
    return dict(ids=ids, main=main, share=np.array(share), touched=touched)
