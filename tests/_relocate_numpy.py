"""fp64 NumPy restatement of the ground relocation of GMTI reports, written from include/sarx_relocate.h.  TEST INFRASTRUCTURE ONLY:
the checker of tests/test_relocate.py and tests/test_gpu_relocate.py.  No sarx import.

relocate       : the records of the header and, per report, the unrounded output-pixel coordinates, h2 and the determinant, so that
                 a test can hold its own inputs clear of the decisions' boundaries
out_slot       : the output slot's bytes from an input report array and its records
image_position : the mirror - where a mover at g with radial speed v_los is imaged: the same circle and line with
                 c = u.V - v_los R - h V_z
scatterer_displacement, mover_peak, physics_figures : the scene, the reference displacement and the bounds that the CPU physics test
                 and the end-to-end test on the device share"""
import functools

import numpy as np

REPORT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("power", "<f8"), ("mean", "<f8"), ("interf_re", "<f8"), ("interf_im", "<f8"),
                         ("mag1", "<f4"), ("mag2", "<f4")])
RECORD_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("shift_x", "<f8"), ("shift_y", "<f8"), ("vx", "<f8"), ("vy", "<f8"), ("rank", "<i4"),
                         ("status", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert REPORT_DTYPE.itemsize == 48 and RECORD_DTYPE.itemsize == 64
OK, NO_SPEED, NO_SOLUTION, OFF_GRID, OVERFLOW = 0, 1, 2, 3, 4
HAS_VELOCITY = 1


def tdbp_grid(scene_size, nx, ny):
    """(x0, y0, dx, dy) of the grid of sarx_tdbp_*"""
    return (-scene_size / 2, -scene_size / 2, scene_size / (nx - 1), scene_size / (ny - 1))


def _track_frame(vel):
    s2 = vel[0] * vel[0] + vel[1] * vel[1]
    vs = np.sqrt(s2)
    a = np.array([vel[0] / vs, vel[1] / vs]) if vs > 0 else np.zeros(2)
    return vs, a, np.array([-a[1], a[0]])


def relocate(ij, v_los, pos_ref, vel_ref, in_grid, out_grid, valid=None, v_along=None):
    """ij [n x 2] (i, j); in_grid (x0, y0, dx, dy); out_grid (x0, y0, dx, dy, nx, ny).  Returns (records, aux) with rank = -1
    everywhere still (out_slot fills it) and aux = dict(fj, fi, h2, det): the unrounded pixel coordinates (x - out_x0) / out_dx + 0.5
    and (y - out_y0) / out_dy + 0.5, h2 and the determinant (NaN where the header does not form them)."""
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    n = len(ij)
    P, V = np.asarray(pos_ref, np.float64), np.asarray(vel_ref, np.float64)
    vs, a, nrm = _track_frame(V)
    rec = np.zeros(n, RECORD_DTYPE)
    rec["rank"] = -1
    aux = {k: np.full(n, np.nan) for k in ("fj", "fi", "h2", "det")}
    x0, y0, dx, dy = in_grid
    ox0, oy0, odx, ody, onx, ony = out_grid
    h = -P[2]
    for r in range(n):
        v = float(v_los[r])
        if (valid is not None and int(valid[r]) != 0) or not np.isfinite(v):
            rec["status"][r] = NO_SPEED
            continue
        qx, qy = x0 + float(ij[r, 1]) * dx, y0 + float(ij[r, 0]) * dy
        wx, wy = qx - P[0], qy - P[1]
        rho2 = wx * wx + wy * wy
        R = np.sqrt(rho2 + h * h)
        with np.errstate(all="ignore"):
            al = (wx * V[0] + wy * V[1] + v * R) / vs if vs > 0 else np.nan
            h2 = rho2 - al * al
        aux["h2"][r] = h2
        if vs == 0 or not rho2 > 0 or not h2 >= 0:
            rec["status"][r] = NO_SOLUTION
            continue
        side = 1.0 if wx * nrm[0] + wy * nrm[1] >= 0 else -1.0
        ux, uy = al * a[0] + side * np.sqrt(h2) * nrm[0], al * a[1] + side * np.sqrt(h2) * nrm[1]
        gx, gy = P[0] + ux, P[1] + uy
        rec["x"][r], rec["y"][r], rec["shift_x"][r], rec["shift_y"][r] = gx, gy, gx - qx, gy - qy
        if v_along is not None and np.isfinite(v_along[r]):
            ex, ey = ux / R, uy / R
            det = ex * a[1] - ey * a[0]
            aux["det"][r] = det
            with np.errstate(all="ignore"):
                vx, vy = (v * a[1] - ey * float(v_along[r])) / det, (ex * float(v_along[r]) - a[0] * v) / det
            if det != 0 and np.isfinite(vx) and np.isfinite(vy):
                rec["vx"][r], rec["vy"][r], rec["flags"][r] = vx, vy, HAS_VELOCITY
        fj, fi = (gx - ox0) / odx + 0.5, (gy - oy0) / ody + 0.5
        aux["fj"][r], aux["fi"][r] = fj, fi
        rec["status"][r] = OK if 0 <= np.floor(fj) < onx and 0 <= np.floor(fi) < ony else OFF_GRID
    return rec, aux


def out_slot(reports, rec, aux, max_detections):
    """The output slot's bytes (header, kept reports sorted by (io, jo, r), zeros behind) and the records with their ranks."""
    reports = np.asarray(reports, REPORT_DTYPE)
    rec = rec.copy()
    kept = np.flatnonzero(rec["status"] == OK)
    io, jo = np.floor(aux["fi"][kept]).astype(np.int64), np.floor(aux["fj"][kept]).astype(np.int64)
    order = np.lexsort((kept, jo, io))
    out = reports[kept[order]].copy()
    out["i"], out["j"] = io[order], jo[order]
    rec["rank"][kept[order]] = np.arange(len(kept))
    raw = np.zeros(16 + 48 * max_detections, np.uint8)
    raw[:4].view("<u4")[0] = len(kept)
    raw[16:16 + out.nbytes] = out.view(np.uint8)
    return raw, rec


def overflow_outputs(count, max_detections):
    """What an unusable input slot gives: record 0 with the status alone, and the output header (count carried, overflow = 1)."""
    rec = np.zeros(1, RECORD_DTYPE)
    rec["status"] = OVERFLOW
    hdr = np.zeros(16, np.uint8)
    hdr[:8].view("<u4")[:] = (count, 1)
    return rec, hdr


def image_position(g, v_los, pos_ref, vel_ref):
    """(qx, qy): where a mover at ground point g = (gx, gy) with radial speed v_los (receding positive) is imaged, or None when no
    ground point has its range and range rate."""
    P, V = np.asarray(pos_ref, np.float64), np.asarray(vel_ref, np.float64)
    vs, a, nrm = _track_frame(V)
    ux, uy, h = g[0] - P[0], g[1] - P[1], -P[2]
    rho2 = ux * ux + uy * uy
    R = np.sqrt(rho2 + h * h)
    if vs == 0 or not rho2 > 0:
        return None
    al = (ux * V[0] + uy * V[1] - v_los * R) / vs          # u.V - v_los R - h V_z, with u_z = h
    h2 = rho2 - al * al
    if not h2 >= 0:
        return None
    side = 1.0 if ux * nrm[0] + uy * nrm[1] >= 0 else -1.0
    return (P[0] + al * a[0] + side * np.sqrt(h2) * nrm[0], P[1] + al * a[1] + side * np.sqrt(h2) * nrm[1])


def circle_geometry(angle_deg, radius=5000.0, height=3000.0, speed=100.0):
    """(pos, vel) of a platform on a circle of `radius` at `height` around the scene centre, flying counter-clockwise."""
    t = np.deg2rad(angle_deg)
    return (np.array([radius * np.cos(t), radius * np.sin(t), height]), np.array([-speed * np.sin(t), speed * np.cos(t), 0.0]))


# ---- the physics on the three-receiver scene of tests/_tdbp_multi_numpy.py ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scatterer_displacement():
    """(b, pixel): where the restated back-projection images a stationary scatterer alone at (0, 0) on GRID with the pulse ranges of
    the three-receiver scene - the image's own range placement and pixel quantisation, not the relocation's."""
    import _tdbp_multi_numpy as mref
    from oracle import tdbp_oracle as tb
    size, nx, ny = mref.GRID
    sc = mref.scene(320, tb.scaled_constants(), [(0.0, 0.0, 50.0)], [], mref.OFFSETS_3[:2])
    img = mref.stack_images(sc, size, nx, ny, mref.FIRST_3[:2], mref.N_USED)
    i, j = np.unravel_index(np.argmax(np.abs(img[0])), img[0].shape)
    x0, y0, dx, dy = tdbp_grid(size, nx, ny)
    return np.array([x0 + j * dx, y0 + i * dy]), (int(i), int(j))


def mover_peak(img):
    """(i, j) of the peak of |I0 - I1|"""
    d = np.abs(np.asarray(img[0]) - np.asarray(img[1]))
    return tuple(int(x) for x in np.unravel_index(np.argmax(d), d.shape))


def physics_figures(vy, peak, g, v_rec, v_true, P, V, b):
    """For the mover of three_rx_scene(vy) found at pixel `peak` and relocated to g with the speed v_rec: err = |(g - truth) - b| per
    axis; bound = one pixel spacing of the axis (two half-pixel quantisations: the mover's peak and the scatterer's), on the
    along-track axis (x on this arc) R / |V_xy| |v_rec - v_true| more; before = the same quantity without relocation."""
    import _tdbp_multi_numpy as mref
    size, nx, ny = mref.GRID
    x0, y0, dx, dy = tdbp_grid(size, nx, ny)
    truth = np.array([49.5 * vy, 0.0])
    q = np.array([x0 + peak[1] * dx, y0 + peak[0] * dy])
    R = float(np.linalg.norm(np.array([q[0], q[1], 0.0]) - np.asarray(P)))
    slope = R / float(np.hypot(V[0], V[1]))
    spacing = np.array([dx, dy])
    return dict(err=np.abs((np.asarray(g, np.float64) - truth) - b), bound=spacing + np.array([slope * abs(v_rec - v_true), 0.0]),
                before=np.abs((q - truth) - b), slope=slope, spacing=spacing, truth=truth, g=np.asarray(g, np.float64), peak=peak, v_rec=v_rec,
                v_true=v_true)


def physics_line(f):
    return (f"peak {f['peak']}: v_los {f['v_rec']:.3f} against {f['v_true']:.3f} m/s, R / V {f['slope']:.1f} s; relocated to "
            f"({f['g'][0]:.2f}, {f['g'][1]:.2f}) m against ({f['truth'][0]:.0f}, {f['truth'][1]:.0f}); error less b ({f['err'][0]:.2f}, "
            f"{f['err'][1]:.2f}) m within ({f['bound'][0]:.2f}, {f['bound'][1]:.2f}); unrelocated ({f['before'][0]:.1f}, {f['before'][1]:.2f}) m")


def slot_bytes(reports, max_detections, count=None, overflow=0):
    """A GMTI slot as bytes: header (count, overflow, 0, 0), the reports, zeros up to max_detections reports."""
    reports = np.asarray(reports, REPORT_DTYPE)
    raw = np.zeros(16 + 48 * max_detections, np.uint8)
    raw[:8].view("<u4")[:] = (len(reports) if count is None else count, overflow)
    k = min(len(reports), max_detections)
    raw[16:16 + 48 * k] = reports[:k].view(np.uint8)
    return raw


# ---- the VideoSAR scenario of the tracker tests -----------------------------------------------------------------------------
VIDEO = dict(n_frames=16, step_deg=5.0, dt=2.0, speed=10.0, heading_deg=160.0, start=(-150.0, -40.0), n_false=4, missed=(5, 11),
             grid=(1022.0, 512, 512),                                     # the image: 512 x 512 pixels of 2 m
             out_grid=(-1024.0, -1024.0, 8.0, 8.0, 256, 256),             # the tracker's ground grid: 256 x 256 pixels of 8 m
             max_detections=16, seed=7)


def video_scenario(**kw):
    """16 frames from the 5 km circle at 3 km height, the platform stepping 5 degrees per frame (so its speed is the arc over dt); one
    mover with a steady ground velocity of 10 m/s, not detected in the frames `missed`, imaged at the pixel of
    image_position(g_f, v_los_f) of the 512 x 512 image of 2 m pixels, plus 4 false reports per frame at seeded pixels with seeded
    speeds.  Per frame: reports sorted by (i, j), v_los per report, (P, V), and the index of the mover's report or -1."""
    import _track_numpy as tref
    c = dict(VIDEO, **kw)
    rng = np.random.default_rng(c["seed"])
    x0, y0, dx, dy = tdbp_grid(*c["grid"])
    nx, ny = c["grid"][1:]
    speed = 5000.0 * np.deg2rad(c["step_deg"]) / c["dt"]
    u = c["speed"] * np.array([np.cos(np.deg2rad(c["heading_deg"])), np.sin(np.deg2rad(c["heading_deg"]))])
    frames = []
    for f in range(c["n_frames"]):
        P, V = circle_geometry(20.0 + c["step_deg"] * f, speed=speed)
        g = np.asarray(c["start"]) + u * c["dt"] * f
        los = np.array([g[0] - P[0], g[1] - P[1], -P[2]])
        v_m = float(u @ los[:2] / np.linalg.norm(los))
        q = image_position(g, v_m, P, V)
        cells, speeds = [], []
        if f not in c["missed"]:
            cells.append((int(np.rint((q[1] - y0) / dy)), int(np.rint((q[0] - x0) / dx))))
            speeds.append(v_m)
        for _ in range(c["n_false"]):
            cells.append((int(rng.integers(0, ny)), int(rng.integers(0, nx))))
            speeds.append(float(rng.uniform(-8.0, 8.0)))
        assert len(set(cells)) == len(cells) and all(0 <= i < ny and 0 <= j < nx for i, j in cells)
        order = sorted(range(len(cells)), key=lambda k: cells[k])
        rep = tref.make_reports([cells[k] for k in order], rng)
        assert [(int(a), int(b)) for a, b in zip(rep["i"], rep["j"])] == [cells[k] for k in order]
        frames.append(dict(reports=rep, v_los=np.array([speeds[k] for k in order]), P=P, V=V, g=g,
                           mover=order.index(0) if f not in c["missed"] else -1))
    gate = float(np.ceil(3.0 * c["speed"] * c["dt"] / c["out_grid"][2]))      # the mover's step plus two pixels of quantisation
    return c, frames, gate


def relocate_video(c, frames):
    """The restatement's relocated slots of a scenario: per frame (slot bytes, records, aux)."""
    grid = tdbp_grid(*c["grid"])
    out = []
    for fr in frames:
        rec, aux = relocate(np.stack([fr["reports"]["i"], fr["reports"]["j"]], 1), fr["v_los"], fr["P"], fr["V"], grid, c["out_grid"])
        raw, rec = out_slot(fr["reports"], rec, aux, c["max_detections"])
        out.append((raw, rec, aux))
    return out


# ---- the seeded report lists of the parity and guard tests --------------------------------------------------------------------------
CASE_GRID = (1022.0, 512, 512)                                  # the image: 2 m pixels
CASE_OUT = (-700.0, 250.0, 3.0, -3.5, 300, 260)                 # the output pixels: rows fall as y rises (a negative step)


def seeded_case(count, seed, with_valid=True, with_along=True):
    """`count` reports seen from the 5 km circle: movers at seeded ground points with seeded speeds, imaged at the pixel of
    image_position; every ninth report repeats the pixel and speed of an earlier one (the same output pixel twice), and by turns a
    report gets no finite speed, a non-zero valid word, a speed no ground point has (500 m/s), or a position off the output grid.
    Returns dict(reports, v_los, valid, v_along, P, V); valid / v_along None when not asked for."""
    rng = np.random.default_rng(seed)
    P, V = circle_geometry(rng.uniform(0, 360), speed=rng.uniform(80, 200))
    x0, y0, dx, dy = tdbp_grid(*CASE_GRID)
    rep = np.zeros(count, REPORT_DTYPE)
    v = np.zeros(count)
    valid = np.zeros(count, np.uint32)
    for r in range(count):
        if r % 9 == 8:
            k = int(rng.integers(0, r))
            rep["i"][r], rep["j"][r], v[r] = rep["i"][k], rep["j"][k], v[k]
            continue
        far = r % 11 == 7
        g = rng.uniform(900, 1500, 2) * rng.choice([-1, 1], 2) if far else rng.uniform(-600, 200, 2)
        v[r] = rng.uniform(-9, 9)
        q = image_position(g, v[r], P, V)
        rep["i"][r], rep["j"][r] = int(np.rint((q[1] - y0) / dy)), int(np.rint((q[0] - x0) / dx))     # off the image too: any int is a pixel
        if r % 13 == 3:
            v[r] = (np.nan, np.inf, -np.inf)[r % 3]
        elif r % 13 == 6:
            valid[r] = (1, 3, 0x80000000)[r % 3]
        elif r % 13 == 10:
            v[r] = 500.0
    for f in ("power", "mean", "interf_re", "interf_im"):
        rep[f] = rng.standard_normal(count)
    rep["mag1"], rep["mag2"] = rng.standard_normal(count), rng.standard_normal(count)
    along = rng.uniform(-12, 12, count)
    along[rng.random(count) < 0.2] = np.nan
    return dict(reports=rep, v_los=v, valid=valid if with_valid else None, v_along=along if with_along else None, P=P, V=V)


def expected(case, max_detections):
    """(slot bytes, records, aux) of a seeded case by the restatement, after holding the case clear of every decision boundary: no
    unrounded output-pixel coordinate within 1e-6 of a .5 boundary, no h2 within 1e-6 relative of zero, no determinant within 1e-6
    of zero.  A condition on the inputs: it leaves no report out."""
    rep = case["reports"]
    rec, aux = relocate(np.stack([rep["i"], rep["j"]], 1), case["v_los"], case["P"], case["V"], tdbp_grid(*CASE_GRID), CASE_OUT,
                        valid=case["valid"], v_along=case["v_along"])
    for k in ("fj", "fi"):
        f = aux[k][np.isfinite(aux[k])]
        assert np.all(np.abs(f - np.rint(f)) > 1e-6), k                 # fj = (x - x0) / dx + 0.5: a .5 boundary of the coordinate is an integer fj
    x0, y0, dx, dy = tdbp_grid(*CASE_GRID)
    rho2 = (x0 + rep["j"] * dx - case["P"][0]) ** 2 + (y0 + rep["i"] * dy - case["P"][1]) ** 2
    h2 = aux["h2"]
    assert np.all(np.abs(h2[np.isfinite(h2)]) > 1e-6 * rho2[np.isfinite(h2)])
    det = aux["det"][np.isfinite(aux["det"])]
    assert np.all(np.abs(det) > 1e-6)
    raw, rec = out_slot(rep, rec, aux, max_detections)
    return raw, rec, aux
