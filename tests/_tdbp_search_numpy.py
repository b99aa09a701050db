"""NumPy restatement of the back-projection's focus-velocity search (include/sarx_tdbp_search.h).  TEST INFRASTRUCTURE ONLY.

The image of a hypothesis is oracle.tdbp_oracle.tdbp(..., vel_focus=v_h, rc_data=rc) with rc computed once; the figures are
fp64 sums over P = re^2 + im^2 with the header's tie rule; the line and the parabola are written out again here, independently
of the package."""
import numpy as np

from oracle import tdbp_oracle as tb

RECORD_DTYPE = np.dtype([("s2", "<f8"), ("s4", "<f8"), ("peak", "<f8"), ("peak_ix", "<i4"), ("peak_iy", "<i4")])
MAX_HYP = 1024


def power(img):
    img = np.asarray(img, dtype=np.complex128)
    return img.real * img.real + img.imag * img.imag          # two rounded products, one rounded sum


def metrics(img):
    """(s2, s4, peak, peak_ix, peak_iy) of one image; of equal maxima the smaller iy * nx + ix."""
    p = power(img)
    flat = int(np.argmax(p.ravel()))                          # numpy.argmax: the first of equal maxima in C order
    return float(p.sum()), float((p * p).sum()), float(p.ravel()[flat]), flat % p.shape[1], flat // p.shape[1]


def stack_images(sc, hyps, nx, ny, rc=None):
    """[n_hyp x ny x nx] complex128 of a tdbp_scene dict under every hypothesis; the pulses are compressed once."""
    raw = sc["raw"].astype(np.complex64)
    if rc is None:
        rc = tb.range_compress(raw, sc["num_samples"], sc["k"])
    return np.stack([tb.tdbp(raw, sc["pos"], sc["vel"], sc["t_start"], sc["num_samples"], np.asarray(v, dtype=np.float64), sc["t_vec"],
                             sc["swath"], nx, ny, sc["k"], rc_data=rc) for v in hyps])


def records(stack):
    out = np.zeros(len(stack), dtype=RECORD_DTYPE)
    for h, img in enumerate(stack):
        out[h] = metrics(img)
    return out


def velocity_line(center, direction, half_span, n):
    assert n % 2 == 1
    u = np.asarray(direction, dtype=np.float64) / np.sqrt(np.sum(np.square(np.asarray(direction, dtype=np.float64))))
    return np.array([np.asarray(center, dtype=np.float64) + (half_span * (2.0 * k / (n - 1) - 1.0) if n > 1 else 0.0) * u for k in range(n)])


def line_estimate(offsets, y):
    """(s*, edge): argmax b; interior: s_b + step * (y- - y+) / (2 (y- - 2 y_b + y+)) clipped to half a step; an end: s_b, True."""
    offsets, y = np.asarray(offsets, dtype=np.float64), np.asarray(y, dtype=np.float64)
    b = int(np.argmax(y))
    if b == 0 or b == len(y) - 1:
        return float(offsets[b]), True
    step = offsets[1] - offsets[0]
    den = y[b - 1] - 2.0 * y[b] + y[b + 1]
    d = 0.0 if den == 0.0 else 0.5 * (y[b - 1] - y[b + 1]) / den
    return float(offsets[b] + step * min(max(d, -0.5), 0.5)), False


def recovery_scene():
    """The scene DESIGN.md 4.17 quotes: 2048 pulses of the scaled radar, three scatterers moving at 15 m/s heading 30 degrees."""
    return tb.tdbp_scene(n_pulses=2048, seed=3, k=tb.scaled_constants(), speed=15.0, heading_deg=30.0, swath=72.0, n_targets=3)


RECOVERY_NX = RECOVERY_NY = 24
RECOVERY_OFFSETS = np.arange(-12.0, 12.5, 3.0)                # nine hypotheses along x (the platform's along-track direction)


def recovery_hyps(sc):
    return sc["v_tgt"][None, :] + RECOVERY_OFFSETS[:, None] * np.array([1.0, 0.0, 0.0])[None, :]
