"""fp64 NumPy restatement of the Kalman ground tracker (include/sarx_ktrack.h states the semantics; csrc/ktrack.hip implements them)
- the checker of tests/test_ktrack.py and tests/test_gpu_ktrack.py - and the seeded scenes both use.  No sarx import.

Every fp64 value is formed by the operations the header lists, in its order, one rounding each (NumPy fuses nothing; an array
operation is the scalar operation per element), so the restatement and the kernels make the same decisions."""
import numpy as np

REPORT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("power", "<f8"), ("mean", "<f8"), ("interf_re", "<f8"), ("interf_im", "<f8"),
                         ("mag1", "<f4"), ("mag2", "<f4")])
RECORD_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("shift_x", "<f8"), ("shift_y", "<f8"), ("vx", "<f8"), ("vy", "<f8"), ("rank", "<i4"),
                         ("status", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
HEADER_DTYPE = np.dtype([("n_live", "<u4"), ("n_confirmed", "<u4"), ("next_id", "<i4"), ("frames_done", "<u4"), ("births_total", "<u4"),
                         ("drops_total", "<u4"), ("error", "<u4"), ("error_frame", "<i4"), ("max_tracks", "<u4"), ("reserved0", "<u4"),
                         ("t_last", "<f8"), ("reserved", "<u4", (4,))])
SLOT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("vx", "<f8"), ("vy", "<f8"), ("p", "<f8", (10,)), ("sum_re", "<f8"), ("sum_im", "<f8"),
                       ("sum_power", "<f8"), ("max_ratio", "<f8"), ("nis_last", "<f8"), ("nis_sum", "<f8"), ("id", "<i4"), ("status", "<u4"),
                       ("hits", "<u4"), ("misses", "<u4"), ("age", "<u4"), ("hist", "<u4"), ("last_frame", "<i4"), ("last_report", "<i4")])
assert REPORT_DTYPE.itemsize == 48 and RECORD_DTYPE.itemsize == 64 and HEADER_DTYPE.itemsize == 64 and SLOT_DTYPE.itemsize == 192
FREE, TENTATIVE, CONFIRMED = 0, 1, 2
OK, SLOT_OVERFLOW, TABLE_OVERFLOW, TIME = 0, 1, 2, 3
REC_OK, REC_NO_SPEED, REC_NO_SOLUTION, REC_OFF_GRID, REC_OVERFLOW = 0, 1, 2, 3, 4
HAS_VELOCITY = 1
# p[k] = P[i][j]: the upper triangle row by row
TRI = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (0, 3): 3, (1, 1): 4, (1, 2): 5, (1, 3): 6, (2, 2): 7, (2, 3): 8, (3, 3): 9}

DEFAULTS = dict(sigma_pos=1.0, sigma_v=0.3, sigma_v_tan=10.0, q=0.01, gate_d2=16.27, gate_m=100.0, birth_ratio=0.0, confirm_hits=3,
                confirm_window=5, max_misses=3, max_tracks=1024, max_detections=4096)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def kp(i, j):
    return TRI[(i, j) if i <= j else (j, i)]


def _popcount(x):
    return bin(int(x)).count("1")


def measurements(rec, v_los, P, V, p):
    """Step 3: (usable [n] bool, meas [n x 11] = z_x z_y z_v u_x u_y Rm00 Rm01 Rm11 Rm02 Rm12 Rm22; NaN rows where unusable)."""
    n = len(rec)
    meas = np.full((n, 11), np.nan)
    v = np.asarray(v_los, np.float64)[:n]
    Vx, Vy = float(V[0]), float(V[1])
    s = np.sqrt(Vx * Vx + Vy * Vy)
    with np.errstate(all="ignore"):
        dx, dy = rec["x"] - P[0], rec["y"] - P[1]
        rho2 = dx * dx + dy * dy
        ok = ((rec["status"] == REC_OK) | (rec["status"] == REC_OFF_GRID)) & np.isfinite(v) & np.isfinite(rec["x"]) & np.isfinite(rec["y"]) & \
            (s != 0.0) & (rho2 != 0.0)
        if n == 0 or not ok.any():
            return ok, meas
        ax, ay = Vx / s, Vy / s
        nx, ny = -ay, ax
        R = np.sqrt(rho2 + P[2] * P[2])
        k = R / s
        kax, kay = k * ax, k * ay
        sp2, sv2 = p["sigma_pos"] * p["sigma_pos"], p["sigma_v"] * p["sigma_v"]
        cols = [rec["x"], rec["y"], v, dx / R, dy / R,
                (ax * ax) * sp2 + (nx * nx) * sp2 + (kax * kax) * sv2,
                (ax * ay) * sp2 + (nx * ny) * sp2 + (kax * kay) * sv2,
                (ay * ay) * sp2 + (ny * ny) * sp2 + (kay * kay) * sv2,
                kax * sv2, kay * sv2, np.full(n, sv2)]
    for c, col in enumerate(cols):
        meas[ok, c] = col[ok]
    return ok, meas


def predict(x, P, dt, q):
    """Step 2 on arrays: x [m x 4], P [m x 10] -> (x-, P-)."""
    dt2 = dt * dt
    dt3 = dt2 * dt
    q11, q13, q33 = q * (dt3 / 3.0), q * (dt2 / 2.0), q * dt
    xm = np.stack([x[:, 0] + dt * x[:, 2], x[:, 1] + dt * x[:, 3], x[:, 2], x[:, 3]], axis=1)
    Pm = np.empty_like(P)
    Pm[:, 0] = P[:, 0] + dt * (P[:, 2] + P[:, 2]) + dt2 * P[:, 7] + q11
    Pm[:, 1] = P[:, 1] + dt * (P[:, 3] + P[:, 5]) + dt2 * P[:, 8]
    Pm[:, 2] = P[:, 2] + dt * P[:, 7] + q13
    Pm[:, 3] = P[:, 3] + dt * P[:, 8]
    Pm[:, 4] = P[:, 4] + dt * (P[:, 6] + P[:, 6]) + dt2 * P[:, 9] + q11
    Pm[:, 5] = P[:, 5] + dt * P[:, 8]
    Pm[:, 6] = P[:, 6] + dt * P[:, 9] + q13
    Pm[:, 7] = P[:, 7] + q33
    Pm[:, 8] = P[:, 8]
    Pm[:, 9] = P[:, 9] + q33
    return xm, Pm


def innovation(x, P, m):
    """Step 4 past the coarse box, elementwise on arrays of pairs (x [.. x 4], P [.. x 10], m [.. x 11]) or on single rows: a dict
    with nu [3], c [4], S (the six entries), the factor and d2."""
    ux, uy = m[..., 3], m[..., 4]
    nu = [m[..., 0] - x[..., 0], m[..., 1] - x[..., 1], m[..., 2] - (ux * x[..., 2] + uy * x[..., 3])]
    c = [ux * P[..., 2] + uy * P[..., 3], ux * P[..., 5] + uy * P[..., 6], ux * P[..., 7] + uy * P[..., 8], ux * P[..., 8] + uy * P[..., 9]]
    s00, s01, s11 = P[..., 0] + m[..., 5], P[..., 1] + m[..., 6], P[..., 4] + m[..., 7]
    s02, s12 = c[0] + m[..., 8], c[1] + m[..., 9]
    s22 = (ux * c[2] + uy * c[3]) + m[..., 10]
    with np.errstate(all="ignore"):
        l00 = np.sqrt(s00)
        l10 = s01 / l00
        l20 = s02 / l00
        l11 = np.sqrt(s11 - l10 * l10)
        l21 = (s12 - l20 * l10) / l11
        l22 = np.sqrt((s22 - l20 * l20) - l21 * l21)
        w0 = nu[0] / l00
        w1 = (nu[1] - l10 * w0) / l11
        w2 = ((nu[2] - l20 * w0) - l21 * w1) / l22
        d2 = (w0 * w0 + w1 * w1) + w2 * w2
    return dict(nu=nu, c=c, S=(s00, s01, s11, s02, s12, s22), L=(l00, l10, l20, l11, l21, l22), d2=d2)


def s_matrix(inn):
    s00, s01, s11, s02, s12, s22 = (float(v) for v in inn["S"])
    return np.array([[s00, s01, s02], [s01, s11, s12], [s02, s12, s22]])


def update(x, P, m, inn):
    """Step 6 for one pair (scalars): the new state [4] and P [10]."""
    l00, l10, l20, l11, l21, l22 = (float(v) for v in inn["L"])
    nu = [float(v) for v in inn["nu"]]
    ux, uy = float(m[3]), float(m[4])
    rm = [[m[5], m[6], m[8]], [m[6], m[7], m[9]], [m[8], m[9], m[10]]]
    K = [[0.0] * 3 for _ in range(4)]
    for i in range(4):
        b0, b1, b2 = float(P[kp(i, 0)]), float(P[kp(i, 1)]), float(inn["c"][i])
        y0 = b0 / l00
        y1 = (b1 - l10 * y0) / l11
        y2 = ((b2 - l20 * y0) - l21 * y1) / l22
        K[i][2] = y2 / l22
        K[i][1] = (y1 - l21 * K[i][2]) / l11
        K[i][0] = ((y0 - l10 * K[i][1]) - l20 * K[i][2]) / l00
    xn = np.array([float(x[i]) + ((K[i][0] * nu[0] + K[i][1] * nu[1]) + K[i][2] * nu[2]) for i in range(4)])
    A = [[(1.0 if i == 0 else 0.0) - K[i][0], (1.0 if i == 1 else 0.0) - K[i][1], (1.0 if i == 2 else 0.0) - K[i][2] * ux,
          (1.0 if i == 3 else 0.0) - K[i][2] * uy] for i in range(4)]
    Pn = np.zeros(10)
    for i in range(4):
        M = [((A[i][0] * float(P[kp(0, j)]) + A[i][1] * float(P[kp(1, j)])) + A[i][2] * float(P[kp(2, j)])) + A[i][3] * float(P[kp(3, j)])
             for j in range(4)]
        G = [(K[i][0] * float(rm[0][c]) + K[i][1] * float(rm[1][c])) + K[i][2] * float(rm[2][c]) for c in range(3)]
        for j in range(i, 4):
            T = ((M[0] * A[j][0] + M[1] * A[j][1]) + M[2] * A[j][2]) + M[3] * A[j][3]
            U = (G[0] * K[j][0] + G[1] * K[j][1]) + G[2] * K[j][2]
            Pn[kp(i, j)] = T + U
    return xn, Pn


def birth_state(m, rec, p):
    """Step 9: (state [4], P [10]) of a track born from measurement row m and its record."""
    ux, uy = float(m[3]), float(m[4])
    mm = np.sqrt(ux * ux + uy * uy)
    ex, ey = ux / mm, uy / mm
    emx, emy = ex / mm, ey / mm
    tx, ty = -ey, ex
    P = np.zeros(10)
    P[0], P[1], P[4] = m[5], m[6], m[7]
    P[2], P[3], P[5], P[6] = m[8] * emx, m[8] * emy, m[9] * emx, m[9] * emy
    if int(rec["flags"]) & HAS_VELOCITY:
        vx, vy = float(rec["vx"]), float(rec["vy"])
        P[7], P[8], P[9] = m[10], 0.0, m[10]
    else:
        vr = float(m[2]) / mm
        vx, vy = vr * ex, vr * ey
        sm = p["sigma_v"] / mm
        sm2, st2 = sm * sm, p["sigma_v_tan"] * p["sigma_v_tan"]
        P[7] = sm2 * (ex * ex) + st2 * (tx * tx)
        P[8] = sm2 * (ex * ey) + st2 * (tx * ty)
        P[9] = sm2 * (ey * ey) + st2 * (ty * ty)
    return np.array([float(m[0]), float(m[1]), vx, vy]), P


class Tracker:
    """The table as a header record and a SLOT_DTYPE array; step() is one frame.  `log` keeps, per step, what the guard-band
    assertions of the GPU tests need: every eligible-or-nearly pair's d2 and nu, S's condition numbers, the birth ratios."""

    def __init__(self, p, keep_log=False):
        self.p = p
        self.hdr = np.zeros((), HEADER_DTYPE)
        self.hdr["error_frame"] = -1
        self.hdr["max_tracks"] = p["max_tracks"]
        self.slots = np.zeros(p["max_tracks"], SLOT_DTYPE)
        self.assoc = []
        self.keep_log = keep_log
        self.log = []
        self.nis = []                                            # every matched pair's d2

    def table_bytes(self):
        return np.concatenate([np.frombuffer(self.hdr.tobytes(), np.uint8), self.slots.view(np.uint8)])

    def step(self, reports, rec, v_los, frame, count=None, overflow=0):
        """reports: REPORT_DTYPE of the relocation's input slot; rec: its RECORD_DTYPE records; v_los per report;
        frame = dict(t, P, V, index)."""
        p, h, s = self.p, self.hdr, self.slots
        reports = np.asarray(reports, REPORT_DTYPE)
        rec = np.asarray(rec, RECORD_DTYPE)
        n = len(reports) if count is None else int(count)
        row = np.full(p["max_detections"], -1, np.int32)
        self.assoc.append(row)
        fi = int(frame["index"])
        if h["error"] != OK:
            return row
        if overflow or n > p["max_detections"] or (n >= 1 and len(rec) >= 1 and rec["status"][0] == REC_OVERFLOW):
            h["error"], h["error_frame"] = SLOT_OVERFLOW, fi
            return row
        dt = 0.0 if h["frames_done"] == 0 else float(frame["t"]) - float(h["t_last"])
        if not (dt >= 0.0 and np.isfinite(dt)):
            h["error"], h["error_frame"] = TIME, fi
            return row
        live = np.flatnonzero(s["status"] != FREE)
        xm, Pm = predict(np.stack([s["x"][live], s["y"][live], s["vx"][live], s["vy"][live]], axis=1), s["p"][live], dt, p["q"])
        usable, meas = measurements(rec[:n], v_los, np.asarray(frame["P"], np.float64), np.asarray(frame["V"], np.float64), p)
        best_t = np.full(n, -1)
        best_r = np.full(len(live), -1)
        d2m = None
        log = dict(d2=[], nu=[], cond=[], ratio=[], gaps=[])
        if len(live) and n:
            with np.errstate(invalid="ignore"):
                nux = meas[None, :, 0] - xm[:, None, 0]
                nuy = meas[None, :, 1] - xm[:, None, 1]
                box = (np.abs(nux) <= p["gate_m"]) & (np.abs(nuy) <= p["gate_m"])
            d2m = np.full((len(live), n), np.inf)
            ti, ri = np.nonzero(box)
            if len(ti):
                inn = innovation(xm[ti], Pm[ti], meas[ri])
                d2 = inn["d2"]
                with np.errstate(invalid="ignore"):
                    d2m[ti, ri] = np.where(d2 <= p["gate_d2"], d2, np.inf)
                if self.keep_log:
                    log["d2"] = d2
                    S = np.stack([np.stack([inn["S"][0], inn["S"][1], inn["S"][3]], -1), np.stack([inn["S"][1], inn["S"][2], inn["S"][4]], -1),
                                  np.stack([inn["S"][3], inn["S"][4], inn["S"][5]], -1)], -2)
                    log["cond"] = np.linalg.cond(S)
            if self.keep_log:
                with np.errstate(invalid="ignore"):
                    log["nu"] = np.concatenate([nux[np.isfinite(nux)], nuy[np.isfinite(nuy)]])
                fin = np.where(np.isfinite(d2m), d2m, np.nan)
                for axis in (0, 1):                           # the two best of every report's tracks and of every track's reports
                    if fin.shape[axis] > 1:
                        srt = np.sort(fin, axis=axis)         # NaN (not eligible) last
                        a, b = np.take(srt, 0, axis=axis), np.take(srt, 1, axis=axis)
                        both = np.isfinite(b)
                        log["gaps"] += list((b[both] - a[both]) / b[both])
            br = np.argmin(d2m, axis=1)                       # the first minimum: ties to the smaller r
            best_r = np.where(np.isfinite(d2m[np.arange(len(live)), br]), br, -1)
            bt = np.argmin(d2m, axis=0)                       # rows are in rising slot index: ties to the smaller slot
            best_t = np.where(np.isfinite(d2m[bt, np.arange(n)]), bt, -1)     # an index into `live`
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = reports["power"][:n] / reports["mean"][:n]
        births = [r for r in range(n) if usable[r] and best_t[r] < 0 and (p["birth_ratio"] == 0.0 or ratio[r] >= p["birth_ratio"])]
        if self.keep_log:
            log["ratio"] = ratio[usable[:n]] if n else []
            self.log.append(log)
        win = (1 << p["confirm_window"]) - 1
        drops = 0
        for k, t in enumerate(live):
            r = int(best_r[k])
            matched = r >= 0 and best_t[r] == k
            x = s[t]
            if matched:
                z = reports[r]
                inn = innovation(xm[k], Pm[k], meas[r])
                xn, Pn = update(xm[k], Pm[k], meas[r], inn)
                x["x"], x["y"], x["vx"], x["vy"] = xn
                x["p"] = Pn
                d2 = float(inn["d2"])
                self.nis.append(d2)
                x["nis_last"] = d2
                x["nis_sum"] += d2
                x["hits"] += 1
                x["misses"], x["last_frame"], x["last_report"] = 0, fi, r
                x["sum_re"] += z["interf_re"]
                x["sum_im"] += z["interf_im"]
                x["sum_power"] += z["power"]
                if ratio[r] > x["max_ratio"]:
                    x["max_ratio"] = ratio[r]
                row[r] = x["id"]
            else:
                x["x"], x["y"], x["vx"], x["vy"] = xm[k]
                x["p"] = Pm[k]
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
            h["error"], h["error_frame"] = TABLE_OVERFLOW, fi
        else:
            for k, r in enumerate(births):
                x = s[free[k]]
                z = reports[r]
                xb, Pb = birth_state(meas[r], rec[r], p)
                x["x"], x["y"], x["vx"], x["vy"] = xb
                x["p"] = Pb
                x["sum_re"], x["sum_im"], x["sum_power"], x["max_ratio"] = z["interf_re"], z["interf_im"], z["power"], ratio[r]
                x["id"], x["status"], x["hits"], x["age"], x["hist"] = h["next_id"] + k, TENTATIVE, 1, 1, 1
                x["last_frame"], x["last_report"] = fi, r
                row[r] = x["id"]
            made = len(births)
            h["frames_done"] += 1
        h["n_live"] = np.count_nonzero(s["status"] != FREE)
        h["n_confirmed"] = np.count_nonzero(s["status"] == CONFIRMED)
        h["next_id"] += made
        h["births_total"] += made
        h["drops_total"] += drops
        h["t_last"] = frame["t"]
        return row


def run(frames, p, keep_log=False):
    """frames: dicts with reports, rec, v_los, t, P, V and optionally count, overflow.  Returns the Tracker after all steps."""
    tr = Tracker(p, keep_log)
    for f, fr in enumerate(frames):
        tr.step(fr["reports"], fr["rec"], fr["v_los"], dict(t=fr["t"], P=fr["P"], V=fr["V"], index=fr.get("index", f)), fr.get("count"),
                fr.get("overflow", 0))
    return tr


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def circle_geometry(angle_deg, radius=5000.0, height=3000.0, speed=100.0):
    """(pos, vel) of a platform on a circle of `radius` at `height` around the scene centre, flying counter-clockwise."""
    t = np.deg2rad(angle_deg)
    return (np.array([radius * np.cos(t), radius * np.sin(t), height]), np.array([-speed * np.sin(t), speed * np.cos(t), 0.0]))


CIRCLE = dict(step_deg=5.0, dt=2.0, start_deg=20.0)
CIRCLE_SPEED = 5000.0 * np.deg2rad(CIRCLE["step_deg"]) / CIRCLE["dt"]         # 218 m/s: the arc over dt


def frame_geometry(f):
    return circle_geometry(CIRCLE["start_deg"] + CIRCLE["step_deg"] * f, speed=CIRCLE_SPEED)


def make_reports(n, rng=None):
    """n reports as the relocation's input slot carries them: pixels that nobody reads here, power / mean = 20 .. 40."""
    rep = np.zeros(n, REPORT_DTYPE)
    rep["i"], rep["j"] = np.arange(n) // 64, np.arange(n) % 64
    u = rng.random(n) if rng is not None else np.full(n, 0.5)
    rep["mean"] = 1.0
    rep["power"] = 20.0 + 20.0 * u
    ph = rng.uniform(-3, 3, n) if rng is not None else np.zeros(n)
    rep["interf_re"], rep["interf_im"] = rep["power"] * np.cos(ph), rep["power"] * np.sin(ph)
    rep["mag1"] = rep["mag2"] = np.sqrt(rep["power"])
    return rep


def make_records(g, status=None, vel=None):
    """Records at ground positions g [n x 2]; status per record (default OK); vel [n x 2] with NaN rows = no velocity."""
    g = np.asarray(g, np.float64).reshape(-1, 2)
    rec = np.zeros(len(g), RECORD_DTYPE)
    rec["x"], rec["y"] = g[:, 0], g[:, 1]
    rec["rank"] = -1
    if status is not None:
        rec["status"] = status
    if vel is not None:
        vel = np.asarray(vel, np.float64).reshape(-1, 2)
        has = np.isfinite(vel[:, 0])
        rec["vx"][has], rec["vy"][has] = vel[has, 0], vel[has, 1]
        rec["flags"][has] = HAS_VELOCITY
    return rec


def measure(g, vel, P, V, sigma_pos, sigma_v, rng):
    """Measurements of movers at g [n x 2] with ground velocity vel [n x 2]: the independent errors (along-track placement,
    cross-track placement, speed) drawn and mapped through J at the TRUE position - the speed error moves the report k e_v along
    track.  Returns (z_xy [n x 2], v_los [n])."""
    g, vel = np.asarray(g, np.float64), np.asarray(vel, np.float64)
    s = np.hypot(V[0], V[1])
    a = np.array([V[0], V[1]]) / s
    nrm = np.array([-a[1], a[0]])
    d = g - np.asarray(P[:2])
    R = np.sqrt(np.sum(d * d, axis=1) + P[2] * P[2])
    u = d / R[:, None]
    k = R / s
    e = rng.standard_normal((len(g), 3)) * np.array([sigma_pos, sigma_pos, sigma_v])
    z = g + e[:, :1] * a + e[:, 1:2] * nrm + (k * e[:, 2])[:, None] * a
    return z, np.sum(vel * u, axis=1) + e[:, 2]


def mover_scene(n_movers, n_frames, seed, speeds=None, sigma_v_tan=10.0, spacing=250.0, sigma_pos=1.0, sigma_v=0.3):
    """n_movers steady movers that start on a square lattice `spacing` apart around the scene centre, seen from the circle of CIRCLE
    (5 km radius, 3 km height, 5 degrees and 2 s per frame).  Velocities N(0, sigma_v_tan^2 I), or with speeds = (lo, hi) a uniform
    speed in that range at a uniform heading.  Returns (frames for run(), truth dict(g0, vel))."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_movers)))
    ix = np.arange(n_movers)
    g0 = np.stack([(ix % side - (side - 1) / 2.0) * spacing, (ix // side - (side - 1) / 2.0) * spacing], axis=1)
    g0 = g0 + rng.uniform(-20, 20, g0.shape)
    if speeds is None:
        vel = rng.standard_normal((n_movers, 2)) * sigma_v_tan
    else:
        sp, hd = rng.uniform(speeds[0], speeds[1], n_movers), rng.uniform(0, 2 * np.pi, n_movers)
        vel = np.stack([sp * np.cos(hd), sp * np.sin(hd)], axis=1)
    frames = []
    for f in range(n_frames):
        P, V = frame_geometry(f)
        t = CIRCLE["dt"] * f
        z, v = measure(g0 + vel * t, vel, P, V, sigma_pos, sigma_v, rng)
        frames.append(dict(reports=make_reports(n_movers, rng), rec=make_records(z), v_los=v, t=t, P=P, V=V))
    return frames, dict(g0=g0, vel=vel)


# ---- the seeded report lists of the parity and guard tests --------------------------------------------------------------------------
EDGE = dict(q=0.05, gate_d2=16.27, gate_m=60.0, birth_ratio=10.0, max_misses=1, confirm_hits=2, confirm_window=3)


def edge_scene(count, max_tracks, seed, n_frames=4, max_detections=None):
    """`count` reports per frame for a table of max_tracks: K movers (at most max_tracks less a sixteenth) on a lattice 120 m apart, every fifth
    pair of neighbours only 12 m apart (rival tracks, rival reports), measured with noise; every third carries a full velocity in its
    record (the other birth form); mover k with k % 7 == 3 is not seen in frame 2.  The other count - K reports are clutter whose
    power / mean = 5 lies below birth_ratio = 10 - they start nothing, but those dropped within 15 m of a mover compete for its
    track - with every record status and a non-finite speed by turns.  The report order is shuffled per frame.  Returns (frames for
    run(), params)."""
    rng = np.random.default_rng(seed)
    md = max_detections or (count + 5)
    p = params(max_tracks=max_tracks, max_detections=md, **EDGE)
    K = min(count, max(1, max_tracks - max(2, max_tracks // 16)))      # headroom: a rival that coasts is dropped, its mover reborn
    side = int(np.ceil(np.sqrt(max(K, 1))))
    ix = np.arange(K)
    g0 = np.stack([(ix % side - (side - 1) / 2.0) * 120.0, (ix // side - (side - 1) / 2.0) * 120.0], axis=1) + rng.uniform(-10, 10, (K, 2))
    for k in range(1, K, 2):
        if (k // 2) % 5 == 0:
            g0[k] = g0[k - 1] + np.array([9.0, 8.0])
    vel = rng.standard_normal((K, 2)) * 5.0
    span = side * 60.0 + 200.0
    statuses = [REC_OK, REC_NO_SPEED, REC_NO_SOLUTION, REC_OFF_GRID, REC_OK, REC_OFF_GRID]
    frames = []
    for f in range(n_frames):
        P, V = frame_geometry(f)
        t = CIRCLE["dt"] * f
        seen = np.array([not (f == 2 and k % 7 == 3) for k in range(K)], bool)
        z, v = measure(g0 + vel * t, vel, P, V, p["sigma_pos"], p["sigma_v"], rng)
        given = np.where((ix % 3 == 1)[:, None], vel + rng.standard_normal((K, 2)) * 0.3, np.nan)
        n_m = int(seen.sum())
        n_c = count - n_m
        zc = np.empty((n_c, 2))
        vc = rng.uniform(-8, 8, n_c)
        st = np.array([statuses[c % 6] for c in range(n_c)], np.uint32)
        for c in range(n_c):
            if K and c % 2 == 0:
                m = int(rng.integers(0, K))
                zc[c] = z[m] + rng.uniform(-15, 15, 2)
                vc[c] = v[m] + rng.uniform(-0.5, 0.5)
            else:
                zc[c] = rng.uniform(-span, span, 2)
            if c % 6 == 4:
                vc[c] = (np.nan, np.inf, -np.inf)[(c // 6) % 3]
        rec = np.concatenate([make_records(z[seen], vel=given[seen]), make_records(zc, status=st)])
        rep = make_reports(count, rng)
        rep["power"][n_m:] = 5.0
        order = rng.permutation(count)
        frames.append(dict(reports=rep[order], rec=rec[order], v_los=np.concatenate([v[seen], vc])[order], t=t, P=P, V=V))
    return frames, p


def clear_of_boundaries(tr, p, margin=1e-6):
    """The guard-band condition on a run's INPUTS, from the restatement's log (keep_log=True): every d2 against gate_d2, every
    |nu_x|, |nu_y| against gate_m, the gap between the two best eligible d2 of every track and of every report, and every power / mean
    against birth_ratio, each clear by `margin` relative.  Returns the largest condition number of S among the pairs formed."""
    cond = 1.0
    for log in tr.log:
        d2 = np.asarray(log["d2"], np.float64)
        assert np.all(np.isfinite(d2)) and np.all(np.abs(d2 - p["gate_d2"]) > margin * p["gate_d2"])
        nu = np.abs(np.asarray(log["nu"], np.float64))
        assert np.all(np.abs(nu - p["gate_m"]) > margin * p["gate_m"])
        assert np.all(np.asarray(log["gaps"], np.float64) > margin)
        ratio = np.asarray(log["ratio"], np.float64)
        assert np.all(np.abs(ratio - p["birth_ratio"]) > margin * max(p["birth_ratio"], 1.0))
        if len(log["cond"]):
            cond = max(cond, float(np.max(log["cond"])))
    return cond
