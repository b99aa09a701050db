"""NumPy restatement of the GMTI refocus (include/sarx_refocus.h, csrc/refocus.hip): the checker of tests/test_refocus.py and
tests/test_gpu_refocus.py, in fp64 throughout.

Images are in the device layout [n_az x n_rg] (i = azimuth).  For report (i, j): the chip is rows i0 .. i0 + L - 1 with
i0 = clamp(i - L/2, 0, n_az - L) and columns j - W/2 .. j + W/2 (zero outside the image); x = slc1 - slc2 e^{j cal} (DPCA) or slc1.
Hypothesis k: Y_k = ifft(fft(x, axis=0) * H_k, axis=0), H_k(f, c) = exp(j 4 pi R_c / lambda (D(f; V'_k) - D(f; V_r))) on the
f = fftfreq(L, 1/prf) axis, D(f; V) = sqrt(1 - (lambda f / 2V)^2) with negative arguments clamped to 1e-9, R_c = r0 + j_c dr.
S_k = sum |Y_k|^4 / (sum |x|^2)^2 (0 for an all-zero chip); k* = argmax S_k, ties to the smaller k; the peak is the argmax of
|Y_{k*}|^2 over the chip's in-image cells, ties to the smaller linear index."""
import numpy as np


def phase_rate(L, lam, vr, prf, vp):
    """g(f) = 2 (D(f; V') - D(f; V_r)) / lambda in revolutions per metre of range, formed stably, [L] fp64."""
    f = np.fft.fftfreq(L, 1.0 / prf)
    q = 0.25 * lam * lam * f * f
    ar, ap = 1.0 - q / (vr * vr), 1.0 - q / (vp * vp)
    d, dp = np.sqrt(np.where(ar < 0, 1e-9, ar)), np.sqrt(np.where(ap < 0, 1e-9, ap))
    stable = q * (1.0 / (vr * vr) - 1.0 / (vp * vp)) / (dp + d)
    return 2.0 * np.where((ar < 0) | (ap < 0), dp - d, stable) / lam


def filt(L, ranges, lam, vr, prf, vp):
    """H [L x W] for the columns' ranges."""
    rev = phase_rate(L, lam, vr, prf, vp)[:, None] * np.asarray(ranges, np.float64)[None, :]
    return np.exp(2j * np.pi * (rev - np.rint(rev)))


def chip(slc1, slc2, i, j, L, W, source="dpca", cal=0.0):
    """x [L x W] complex128, i0, the chip's column indices and which of them lie inside the image."""
    n_az, n_rg = slc1.shape
    i0 = min(max(i - L // 2, 0), n_az - L)
    cols = np.arange(j - W // 2, j + W // 2 + 1)
    inside = (cols >= 0) & (cols < n_rg)
    x = np.zeros((L, W), np.complex128)
    a = slc1[i0:i0 + L][:, cols[inside]].astype(np.complex128)
    if source == "dpca":
        a = a - slc2[i0:i0 + L][:, cols[inside]].astype(np.complex128) * np.exp(1j * cal)
    x[:, inside] = a
    return x, i0, cols, inside


def sharpness(y, e2):
    return float(np.sum(np.abs(y) ** 4) / (e2 * e2)) if e2 > 0 else 0.0


def refocus_one(slc1, slc2, i, j, L, W, speeds, lam, vr, prf, r0, dr, source="dpca", cal=0.0):
    """Everything the device computes for one report: curve, k*, record fields and Y_{k*}."""
    x, i0, cols, inside = chip(slc1, slc2, i, j, L, W, source, cal)
    e2 = float(np.sum(np.abs(x) ** 2))
    X = np.fft.fft(x, axis=0)
    ranges = r0 + cols * dr
    ys = [np.fft.ifft(X * filt(L, ranges, lam, vr, prf, v), axis=0) for v in speeds]
    curve = np.array([sharpness(y, e2) for y in ys])
    k = int(np.argmax(curve))                          # first maximum: ties to the smaller k
    y = ys[k]
    p = np.abs(y) ** 2
    p[:, ~inside] = -1.0
    m, c = np.unravel_index(int(np.argmax(p)), p.shape)   # row-major first maximum = smallest linear image index
    n = len(speeds)
    return dict(curve=curve, k_best=k, i0=i0, peak_i=int(i0 + m), peak_j=int(cols[c]), s_best=curve[k],
                s_prev=curve[k - 1] if k > 0 else -1.0, s_next=curve[k + 1] if k + 1 < n else -1.0,
                s_identity=sharpness(x, e2), peak_power=float(p[m, c]), orig_power=float(np.max(np.abs(x) ** 2)), chip=y)


def refocus(slc1, slc2, positions, L, W, speeds, lam, vr, prf, r0, dr, source="dpca", cal=0.0):
    return [refocus_one(slc1, slc2, int(i), int(j), L, W, speeds, lam, vr, prf, r0, dr, source, cal) for i, j in positions]


def smear(img, i, j, L, W, lam, vr, prf, r0, dr, vp):
    """The inverse of hypothesis vp on the chip around (i, j): conj(H) applied to the image's chip in place (what a mover whose
    true compression speed is vp looks like after the stationary filter).  Returns i0."""
    n_az, n_rg = img.shape
    i0 = min(max(i - L // 2, 0), n_az - L)
    cols = np.arange(j - W // 2, j + W // 2 + 1)
    cols = cols[(cols >= 0) & (cols < n_rg)]
    sub = img[i0:i0 + L][:, cols].astype(np.complex128)
    h = filt(L, r0 + cols * dr, lam, vr, prf, vp)
    img[i0:i0 + L, cols] = np.fft.ifft(np.fft.fft(sub, axis=0) * np.conj(h), axis=0)
    return i0
