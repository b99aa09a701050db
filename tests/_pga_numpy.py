"""NumPy fp64 restatement of the phase-gradient autofocus (include/sarx_pga.h), rule by rule, for tests/test_pga.py and
tests/test_gpu_pga.py.  Nothing here is shared with the device code; the scenes, the injected errors and the guards that keep a
test's inputs away from every discrete choice the fp32 kernels could flip live here too."""
import numpy as np

SIZES = (64, 128, 256, 512, 1024)
RECORD_DTYPE = np.dtype([("s2", "<f8"), ("s4", "<f8"), ("rms_phase", "<f8"), ("n_cols_used", "<i4"), ("n_bins_supported", "<i4")])


# ---- scenes and errors ---------------------------------------------------------------------------------------------------------------
def scene(n_az, n_rg, n_t, seed, target_db=30.0):
    """Unit-variance complex Gaussian clutter and n_t point targets target_db above it, in distinct columns, at random rows and
    phases.  complex64 [n_az x n_rg]."""
    rng = np.random.default_rng(seed)
    img = (rng.standard_normal((n_az, n_rg)) + 1j * rng.standard_normal((n_az, n_rg))) / np.sqrt(2.0)
    cols = rng.choice(n_rg, size=n_t, replace=False)
    rows = rng.integers(0, n_az, size=n_t)
    img[rows, cols] += 10.0 ** (target_db / 20.0) * np.exp(2j * np.pi * rng.random(n_t))
    return img.astype(np.complex64)


def remove_line(phi, mask=None):
    """phi minus its least-squares line over the bins of mask (all bins when None); 0 outside the mask."""
    phi = np.asarray(phi, np.float64)
    m = np.ones(len(phi), bool) if mask is None else np.asarray(mask, bool)
    out = np.zeros_like(phi)
    if m.sum() >= 2:
        x = np.arange(len(phi), dtype=np.float64) - len(phi) // 2
        b, a = np.polyfit(x[m], phi[m], 1)
        out[m] = phi[m] - (a + b * x[m])
    return out


def error(kind, n_az):
    """The injected phase errors of the issue over k (fftshift order), x in [-1, 1] across k, line removed."""
    x = np.linspace(-1.0, 1.0, n_az)
    phi = {"quadratic": 6.0 * x * x, "cubic_sine": 4.0 * (0.6 * x ** 3 + 0.4 * np.sin(3.0 * np.pi * x))}[kind]
    return remove_line(phi)


def apply(img, phi, sign):
    """ifft(fft(img) exp(j sign phi)) along axis 0; phi over k in fftshift order: bin u = (k - L/2) mod L."""
    phi = np.asarray(phi, np.float64)
    w = np.exp(1j * sign * np.fft.ifftshift(phi))
    return np.fft.ifft(np.fft.fft(np.asarray(img, np.complex128), axis=0) * w[:, None], axis=0)


def band_limit(img, fraction):
    """The azimuth spectrum zeroed outside the central `fraction` of the bins k; returns (image, in-band mask over k)."""
    n = img.shape[0]
    k = np.arange(n)
    band = np.abs(k - n // 2) < 0.5 * fraction * n
    spec = np.fft.fft(np.asarray(img, np.complex128), axis=0) * np.fft.ifftshift(band)[:, None]
    return np.fft.ifft(spec, axis=0), band


def sharpness(img):
    p = np.abs(np.asarray(img, np.complex128)) ** 2
    return float((p * p).sum() / p.sum() ** 2)


# ---- the algorithm -------------------------------------------------------------------------------------------------------------------
def estimate(g, half_width, min_contrast, power_floor):
    """One estimate on g [L x n_rg] (complex128).  Returns a dict: phi [L], the record's fields, the discrete choices (rows, used,
    supported) and the margins of each of them (guards)."""
    g = np.asarray(g, np.complex128)
    n, n_rg = g.shape
    p = g.real ** 2 + g.imag ** 2
    r = np.argmax(p, axis=0)                                  # the first maximum: ties go to the smaller row
    pk = p[r, np.arange(n_rg)]
    mean = p.sum(axis=0) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        contrast = np.where(pk > 0, pk / np.where(mean > 0, mean, 1.0), 0.0)
    used = (pk > 0) & (contrast >= min_contrast)
    rows = (np.arange(n)[:, None] + r[None, :]) % n
    w = g[rows, np.arange(n_rg)[None, :]]
    dist = np.minimum(np.arange(n), n - np.arange(n))
    w = np.where((dist <= half_width)[:, None] & used[None, :], w, 0.0)
    G = np.fft.fftshift(np.fft.fft(w, axis=0), axes=0)
    P = (np.abs(G) ** 2).sum(axis=1)
    S = np.zeros(n, np.complex128)
    S[1:] = (G[1:] * np.conj(G[:-1])).sum(axis=1)
    pmax = P.max()
    sup = P > power_floor * pmax
    d = np.zeros(n)
    ok = np.zeros(n, bool)
    ok[1:] = sup[1:] & sup[:-1]
    d[ok] = np.angle(S[ok])
    phi = remove_line(np.cumsum(d), sup) if sup.sum() >= 2 else np.zeros(n)
    n_sup = int(sup.sum())
    # guards: the runner-up of every column's peak, the contrasts against min_contrast, the bins against the floor
    runner = np.sort(p, axis=0)[-2] / np.where(pk > 0, pk, 1.0) if n > 1 else np.zeros(n_rg)
    guards = {"runner_up": float(runner[pk > 0].max()) if (pk > 0).any() else 0.0,
              "contrast": float(np.abs(contrast[pk > 0] / min_contrast - 1.0).min()) if min_contrast > 0 and (pk > 0).any() else np.inf,
              "floor": float(np.abs(P / (power_floor * pmax) - 1.0).min()) if power_floor > 0 and pmax > 0 else np.inf,
              "wrap": float(np.pi - np.abs(d).max())}
    return {"phi": phi, "s2": float(p.sum()), "s4": float((p * p).sum()), "rms_phase": float(np.sqrt((phi[sup] ** 2).mean())) if n_sup >= 2 else 0.0,
            "n_cols_used": int(used.sum()), "n_bins_supported": n_sup, "rows": r, "used": used, "supported": sup, "guards": guards}


def pga(img, half_widths, min_contrast=0.0, power_floor=0.0):
    """The whole call on one frame: n_iter = len(half_widths) estimate-and-apply rounds and the final estimate.  Returns
    (out complex128, phi_tot, records RECORD_DTYPE [n_iter + 1], guards: the worst margin of each kind over every estimate,
    supported: the bins supported in every estimate)."""
    g0 = np.asarray(img, np.complex128)
    n_iter = len(half_widths)
    phi_tot = np.zeros(g0.shape[0])
    rec = np.zeros(n_iter + 1, RECORD_DTYPE)
    guards = {"runner_up": 0.0, "contrast": np.inf, "floor": np.inf, "wrap": np.inf}
    supported = np.ones(g0.shape[0], bool)
    g = g0
    for it in range(n_iter + 1):
        e = estimate(g, half_widths[min(it, n_iter - 1)], min_contrast, power_floor)
        rec[it] = (e["s2"], e["s4"], e["rms_phase"], e["n_cols_used"], e["n_bins_supported"])
        guards["runner_up"] = max(guards["runner_up"], e["guards"]["runner_up"])
        for k in ("contrast", "floor", "wrap"):
            guards[k] = min(guards[k], e["guards"][k])
        supported &= e["supported"]
        if it < n_iter:
            phi_tot = phi_tot + e["phi"]
            g = apply(g0, phi_tot, -1)
    return g, phi_tot, rec, guards, supported


def guards_hold(guards):
    """The conditions of the issue: runner-up <= (1 - 1e-4) peak, no contrast within 1 % of min_contrast, no P / max P within 1 % of
    the floor; and no phase step within 0.1 rad of the +-pi wrap."""
    return guards["runner_up"] <= 1.0 - 1e-4 and guards["contrast"] >= 0.01 and guards["floor"] >= 0.01 and guards["wrap"] >= 0.1


def default_half_widths(n_az, n_iter):
    return [max(3, (n_az // 4) >> it) for it in range(n_iter)]


# ---- the cases of the issue, computed once per process ------------------------------------------------------------------------------
N_ITER = 5
KINDS = ("quadratic", "cubic_sine")
CONTRASTS = (0.0, 12.0)
MAIN_SHAPES = [(64, 24, 8), (128, 40, 12), (256, 33, 10), (512, 20, 8)]            # (L, n_rg, n_t)
EXTRA_SHAPES = [(128, 17, 6), (64, 1, 1), (1024, 9, 4)]                             # the GPU tests' further shapes
BAND, BAND_FLOOR = 0.4, 0.05
# the seed of a case is 1 unless listed: the smallest seed whose restatement meets guards_hold (tests/test_pga.py fails on the
# guards when a seed is bad)
SEEDS = {(64, "quadratic", 12.0): 3, (256, "cubic_sine", 12.0): 2}
BAND_SEEDS = {(256, "quadratic"): 2, (256, "cubic_sine"): 3}
FULL_CASES = [(s, k, c) for s in MAIN_SHAPES for k in KINDS for c in CONTRASTS]
BAND_CASES = [(s, k) for s in MAIN_SHAPES for k in KINDS]
EXTRA_CASES = [(s, "cubic_sine", 0.0) for s in EXTRA_SHAPES]
_cache = {}


def case(shape, kind, min_contrast=0.0, band=False):
    """One case, computed once: the unblurred scene, the injected error, the blurred complex64 input and the restatement's result
    on it (out, phi_tot, records, guards, supported), the parameters, and for a band-limited case the in-band mask."""
    key = (tuple(shape), kind, float(min_contrast), bool(band))
    if key not in _cache:
        n_az, n_rg, n_t = shape
        seed = BAND_SEEDS.get((n_az, kind), 1) if band else SEEDS.get((n_az, kind, float(min_contrast)), 1)
        clean = scene(n_az, n_rg, n_t, seed)
        mask = None
        if band:
            clean, mask = band_limit(clean, BAND)
        err = error(kind, n_az)
        blur = apply(clean, err, +1).astype(np.complex64)
        hw = default_half_widths(n_az, N_ITER)
        floor = BAND_FLOOR if band else 0.0
        out, phi, rec, guards, sup = pga(blur, hw, min_contrast, floor)
        _cache[key] = {"clean": clean, "err": err, "blur": blur, "half_widths": hw, "min_contrast": float(min_contrast), "power_floor": floor,
                       "out": out, "phi": phi, "records": rec, "guards": guards, "supported": sup, "band": mask}
    return _cache[key]


def case_id(shape, kind, min_contrast=None):
    return f"{shape[0]}x{shape[1]}-{kind}" + ("" if min_contrast is None else f"-c{min_contrast:g}")
