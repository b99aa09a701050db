#!/usr/bin/env python3
"""GMTI plot extraction timings on the GPU (include/sarx_cluster.h): one sarx_cluster_step_dev at n = 64, 1024, 4096 and 16384
reports in three regimes - singletons (a 12-pixel grid, nothing links), 27 objects of n / 27 members each on sidelobe crosses (a
range arm and an azimuth arm, a report every second pixel), and the dense 64 x 64 block that is one plot of 4096 members (the
serial reduction's worst case) - a 64-frame sarx_cluster_run_dev at n = 1024, and the CFAR launch at 8192^2 in the same process as
the yardstick.  HIP events, medians of rounds.

    python3 tools/bench_cluster.py [--rounds 5] [--reps 20] [--out FILE.json]

The slots have the capacity the case needs (n reports; up to 4096 the kernel keeps the keys in LDS, above that it reads them from
the slot), and the 1024-report cases are timed once more in a slot of 16384, the capacity the C3 batch test uses.  link = (3, 5).
Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))
LINK = (3, 5)


def _reports(cells, seed=1):
    from sarx import gmti
    cells = np.unique(np.asarray(cells, np.int64).reshape(-1, 2), axis=0)          # sorted by (i, j), no cell twice
    rep = np.zeros(len(cells), gmti.REPORT_DTYPE)
    rep["i"], rep["j"] = cells[:, 0], cells[:, 1]
    rng = np.random.default_rng(seed)
    rep["mean"], rep["power"] = 1.0, 30.0 + rng.random(len(cells))
    rep["interf_re"], rep["interf_im"] = rep["power"], 0.0
    return rep


def singletons(n):
    side = int(np.ceil(np.sqrt(n)))
    idx = np.arange(n)
    return _reports(np.stack([12 * (idx // side) + 8, 12 * (idx % side) + 8], axis=1))


def crosses(n, objects=27):
    m = max(n // objects, 1)
    pitch = 2 * m + 40                                     # arms of at most m pixels: neighbours stay apart
    cells = []
    for o in range(objects):
        ci, cj = pitch * (o // 6) + m + 20, pitch * (o % 6) + m + 20
        half = m // 2
        cells += [[ci, cj + 2 * (k - half // 2)] for k in range(half)]
        cells += [[ci + 2 * (k - (m - half) // 2), cj] for k in range(m - half)]
    return _reports(cells)


def dense(n=4096):
    side = int(np.sqrt(n))
    return _reports([[100 + i, 200 + j] for i in range(side) for j in range(side)])


def _median_ms(ctx, fn, rounds, reps):
    fn()
    ctx.sync()
    t = []
    for _ in range(rounds):
        ctx.record(0)
        for _ in range(reps):
            fn()
        ctx.record(1)
        ctx.sync()
        t.append(ctx.elapsed_ms(0, 1) / reps)
    return round(float(np.median(t)), 5), [round(x, 5) for x in t]


def time_step(ctx, rep, link, rounds, reps, capacity=None):
    import sarx
    from sarx import cluster as K, track
    md = capacity or len(rep)
    cp = sarx.ClusterParams(link=link).c_params(md)
    bufs = [ctx.to_device(track.encode_slot(rep, md)), ctx.alloc(K.slot_bytes(md)), ctx.alloc(K.plots_bytes(cp)), ctx.alloc(md * 4)]
    d_in, d_out, d_plots, d_labels = bufs
    med, per = _median_ms(ctx, lambda: K.enqueue_step(ctx, cp, d_in.ptr, d_out.ptr, d_plots.ptr, d_labels.ptr), rounds, reps)
    n_plots = int(d_out.download(np.uint32, (4,))[0])
    largest = int(d_plots.download(np.uint8, (64 * max(n_plots, 1),)).view(K.PLOT_DTYPE)["n_members"].max()) if n_plots else 0
    for b in bufs:
        b.release()
    return {"reports": len(rep), "capacity": md, "plots": n_plots, "largest_plot": largest, "step_ms_median": med, "step_ms_rounds": per}


def time_run(ctx, rep, link, n_frames, rounds, reps):
    import sarx
    from sarx import cluster as K, track
    md = len(rep)
    cp = sarx.ClusterParams(link=link).c_params(md)
    one = track.encode_slot(rep, md)
    bufs = [ctx.to_device(np.tile(one, (n_frames, 1))), ctx.alloc(n_frames * one.size), ctx.alloc(n_frames * K.plots_bytes(cp)),
            ctx.alloc(n_frames * md * 4)]
    d_in, d_out, d_plots, d_labels = bufs
    med, per = _median_ms(ctx, lambda: K.enqueue_run(ctx, cp, d_in.ptr, one.size, d_out.ptr, one.size, n_frames, d_plots.ptr,
                                                     K.plots_bytes(cp), d_labels.ptr), rounds, max(reps // 4, 1))
    for b in bufs:
        b.release()
    return {"frames": n_frames, "reports": md, "run_ms_median": med, "run_ms_rounds": per, "ms_per_frame": round(med / n_frames, 5)}


def time_cfar(ctx, n, rounds, reps):
    """The detector's CFAR launch on an [n x n] noise magnitude plane: the per-frame cost the cluster step stands beside."""
    import sarx
    p = sarx.GmtiParams()
    cp = p.c_params()
    px = n * n
    s = ctx.alloc(px * 8)
    ctx.fill_noise(s, px, 3)
    mag = ctx.alloc(px * 4)
    sarx._ffi.check(ctx.lib.sarx_magnitude_dev(ctx.h, s.ptr, mag.ptr, px), ctx.h)
    slot = ctx.alloc(p.slot_bytes())
    med, per = _median_ms(ctx, lambda: sarx._ffi.check(ctx.lib.sarx_gmti_cfar_dev(ctx.h, mag.ptr, n, n, C.byref(cp), slot.ptr + 16, slot.ptr),
                                                       ctx.h), rounds, reps)
    for b in (s, mag, slot):
        b.release()
    return {"n": n, "cfar_ms_median": med, "cfar_ms_rounds": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    ctx = sarx.default_context()
    sizes = (64, 1024, 4096, 16384)
    out = {"device": ctx.info()["name"], "link": list(LINK),
           "singletons": [time_step(ctx, singletons(n), LINK, a.rounds, a.reps) for n in sizes],
           "objects_27": [time_step(ctx, crosses(n), LINK, a.rounds, a.reps) for n in sizes],
           "dense_block": time_step(ctx, dense(), (2, 2), a.rounds, a.reps),
           "capacity_16384": {"singletons": time_step(ctx, singletons(1024), LINK, a.rounds, a.reps, 16384),
                              "objects_27": time_step(ctx, crosses(1024), LINK, a.rounds, a.reps, 16384)},
           "run": time_run(ctx, crosses(1024), LINK, 64, a.rounds, a.reps),
           "cfar": time_cfar(ctx, 8192, a.rounds, a.reps)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
