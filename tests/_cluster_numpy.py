"""Restatement of the GMTI plot extraction (include/sarx_cluster.h states the semantics; csrc/cluster.hip implements them) - the
checker of tests/test_cluster.py and tests/test_gpu_cluster*.py - by a different algorithm: a breadth-first flood fill over the
n x n link matrix, every pair compared (row r of the matrix is formed whole when r is visited), where the kernel searches sorted
runs and propagates labels.  No sarx import.

Every fp64 value is formed as the header lists it, in Python floats: one addition after another in rising member index, every
product rounded on its own (np.sum would add pairwise), so on finite inputs the restatement and the kernel give the same bits."""
import numpy as np

REPORT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("power", "<f8"), ("mean", "<f8"), ("interf_re", "<f8"), ("interf_im", "<f8"),
                         ("mag1", "<f4"), ("mag2", "<f4")])
PLOT_DTYPE = np.dtype([("n_members", "<i4"), ("peak_report", "<i4"), ("i_min", "<i4"), ("i_max", "<i4"), ("j_min", "<i4"),
                       ("j_max", "<i4"), ("sum_power", "<f8"), ("centroid_i", "<f8"), ("centroid_j", "<f8"), ("max_ratio", "<f8"),
                       ("reserved", "<u4", (2,))])
assert REPORT_DTYPE.itemsize == 48 and PLOT_DTYPE.itemsize == 64
MAX_LINK, MAX_DETECTIONS = 64, 16384


def make_reports(ij, seed=0, power=None):
    """Reports at the cells `ij` (an (n, 2) array, no cell twice), sorted by (i, j), with seeded powers (exponential, or `power` in
    the order of the SORTED list), means, interferograms of random phase and magnitudes."""
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    order = np.lexsort((ij[:, 1], ij[:, 0]))
    ij = ij[order]
    assert len(ij) < 2 or not np.any((np.diff(ij[:, 0]) == 0) & (np.diff(ij[:, 1]) == 0)), "a cell twice"
    n = len(ij)
    rng = np.random.default_rng(seed)
    rep = np.zeros(n, REPORT_DTYPE)
    rep["i"], rep["j"] = ij[:, 0], ij[:, 1]
    rep["power"] = 20.0 + rng.exponential(30.0, n) if power is None else power
    rep["mean"] = 1.0 + rng.random(n)
    ph = rng.uniform(-np.pi, np.pi, n)
    amp = rep["power"] * rng.uniform(0.5, 1.0, n)
    rep["interf_re"], rep["interf_im"] = amp * np.cos(ph), amp * np.sin(ph)
    rep["mag1"] = np.sqrt(rep["power"]).astype(np.float32)
    rep["mag2"] = (0.9 * np.sqrt(rep["power"])).astype(np.float32)
    return rep


def slot_bytes(reports, max_detections, count=None, overflow=0):
    """A GMTI slot as bytes: header (count, overflow, 0, 0), the reports, zeros up to max_detections reports."""
    reports = np.asarray(reports, REPORT_DTYPE)
    raw = np.zeros(16 + 48 * max_detections, np.uint8)
    raw[:8].view("<u4")[:] = (len(reports) if count is None else count, overflow)
    k = min(len(reports), max_detections)
    raw[16:16 + 48 * k] = reports[:k].view(np.uint8)
    return raw


def components(i, j, link_az, link_rg):
    """comp[r] = number of r's component in the order the flood fill opens them (rising smallest member)."""
    n = len(i)
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    comp = np.full(n, -1, np.int64)
    k = 0
    for seed in range(n):
        if comp[seed] >= 0:
            continue
        comp[seed] = k
        queue = [seed]
        while queue:
            r = queue.pop(0)
            row = (np.abs(i - i[r]) <= link_az) & (np.abs(j - j[r]) <= link_rg)      # row r of the link matrix
            new = np.flatnonzero(row & (comp < 0))
            comp[new] = k
            queue.extend(new.tolist())
        k += 1
    return comp, k


class Result:
    """header: the four uint32 of the output header; reports / plots: the n_plots entries written (None after an overflow);
    labels: all max_detections entries."""

    def __init__(self, header, reports, plots, labels):
        self.header, self.reports, self.plots, self.labels = np.asarray(header, "<u4"), reports, plots, labels
        self.n_plots = 0 if reports is None else len(reports)


def cluster(reports, link_az, link_rg, min_members=1, max_detections=None, count=None, overflow=0):
    reports = np.asarray(reports, REPORT_DTYPE)
    md = max(len(reports), 1) if max_detections is None else int(max_detections)
    assert 0 <= link_az <= MAX_LINK and 0 <= link_rg <= MAX_LINK and min_members >= 1 and 1 <= md <= MAX_DETECTIONS
    n = len(reports) if count is None else int(count)
    labels = np.full(md, -1, np.int32)
    if overflow or n > md:
        return Result((n, 1, 0, 0), None, None, labels)
    rep = reports[:n]
    comp, n_comp = components(rep["i"], rep["j"], link_az, link_rg)
    members = [[] for _ in range(n_comp)]
    for r in range(n):                                    # rising report index
        members[int(comp[r])].append(r)
    made = []
    for mem in members:
        if len(mem) < min_members:
            continue
        z = [rep[r] for r in mem]
        peak, best = mem[0], float(z[0]["power"])
        for r, x in zip(mem[1:], z[1:]):
            if float(x["power"]) > best:
                peak, best = r, float(x["power"])
        sp, sre, sim = float(z[0]["power"]), float(z[0]["interf_re"]), float(z[0]["interf_im"])
        wi, wj = float(z[0]["power"]) * float(z[0]["i"]), float(z[0]["power"]) * float(z[0]["j"])
        mr = float(np.float64(z[0]["power"]) / np.float64(z[0]["mean"]))
        for x in z[1:]:
            sp = sp + float(x["power"])
            sre = sre + float(x["interf_re"])
            sim = sim + float(x["interf_im"])
            wi = wi + float(x["power"]) * float(x["i"])
            wj = wj + float(x["power"]) * float(x["j"])
            ratio = float(np.float64(x["power"]) / np.float64(x["mean"]))
            mr = ratio if ratio > mr else mr
        pl = np.zeros((), PLOT_DTYPE)
        pl["n_members"], pl["peak_report"] = len(mem), peak
        pl["i_min"], pl["i_max"] = min(int(x["i"]) for x in z), max(int(x["i"]) for x in z)
        pl["j_min"], pl["j_max"] = min(int(x["j"]) for x in z), max(int(x["j"]) for x in z)
        pl["sum_power"], pl["max_ratio"] = sp, mr
        pl["centroid_i"] = float(rep[peak]["i"]) if sp == 0.0 else wi / sp
        pl["centroid_j"] = float(rep[peak]["j"]) if sp == 0.0 else wj / sp
        out = rep[peak].copy()
        out["interf_re"], out["interf_im"] = sre, sim
        made.append((peak, mem, out, pl))
    made.sort(key=lambda t: t[0])                          # rising index of the peak
    out_rep, out_pl = np.zeros(len(made), REPORT_DTYPE), np.zeros(len(made), PLOT_DTYPE)
    for k, (_, mem, out, pl) in enumerate(made):
        out_rep[k], out_pl[k] = out, pl
        labels[mem] = k
    return Result((len(made), 0, 0, 0), out_rep, out_pl, labels)


FP64_FIELDS = (("reports", ("power", "mean", "interf_re", "interf_im")), ("plots", ("sum_power", "centroid_i", "centroid_j", "max_ratio")))
INT_FIELDS = (("reports", ("i", "j")), ("plots", ("n_members", "peak_report", "i_min", "i_max", "j_min", "j_max", "reserved")))


def compare(res, header, reports, plots, labels, rtol=1e-12):
    """A device result (header: 16 bytes, reports / plots: at least n_plots records, labels: int32 row or None) against `res`:
    integers, labels and the fp32 magnitudes exactly, fp64 fields to rtol.  Returns whether the records are bit-identical."""
    header = np.ascontiguousarray(header).view(np.uint8)[:16].view("<u4")
    assert header.tolist() == res.header.tolist(), (header.tolist(), res.header.tolist())
    if labels is not None:
        np.testing.assert_array_equal(np.asarray(labels, np.int32), res.labels)
    if res.reports is None:
        return True
    k = res.n_plots
    got = {"reports": np.ascontiguousarray(reports).view(np.uint8).reshape(-1)[:48 * k].view(REPORT_DTYPE),
           "plots": None if plots is None else np.ascontiguousarray(plots).view(np.uint8).reshape(-1)[:64 * k].view(PLOT_DTYPE)}
    want = {"reports": res.reports, "plots": res.plots}
    same = True
    for table, names in INT_FIELDS:
        if got[table] is not None:
            for name in names:
                np.testing.assert_array_equal(got[table][name], want[table][name], err_msg=name)
    np.testing.assert_array_equal(got["reports"]["mag1"], want["reports"]["mag1"])
    np.testing.assert_array_equal(got["reports"]["mag2"], want["reports"]["mag2"])
    for table, names in FP64_FIELDS:
        if got[table] is not None:
            for name in names:
                np.testing.assert_allclose(got[table][name], want[table][name], rtol=rtol, atol=0.0, err_msg=name)
            same &= got[table].tobytes() == want[table].tobytes()
    return same
