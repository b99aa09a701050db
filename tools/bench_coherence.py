#!/usr/bin/env python3
"""Sliding-window coherence timings on the GPU (include/sarx_coherence.h): the pair launch at 8192^2 and 16384^2 for several
windows, with coh alone and with igram + mask (+ the summary's finish launch), timed with HIP events in rounds.  The balance
estimate (the same 16 B per pixel read) and the CFAR launch (the same tile-plus-halo shape) are timed in the same process for
comparison.

    python3 tools/bench_coherence.py [--sizes 8192 16384] [--windows 1,1 4,4 16,16] [--rounds 5] [--reps 20] [--out FILE.json]

The images are two device-filled complex noise planes.  Each figure comes with the bytes the launch has to move (20 B per pixel,
29 B with igram and mask), the time those bytes take at COPY_TBPS (the best copy this part reaches, README) and the fraction of that
floor the launch achieves.  Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))

COPY_TBPS = 6.0


def time_launches(ctx, n, windows, rounds, reps):
    import sarx
    from sarx import balance as B
    from sarx import gmti
    K = importlib.import_module("sarx.coherence")
    px = n * n
    s1, s2 = ctx.alloc(px * 8), ctx.alloc(px * 8)
    ctx.fill_noise(s1, px, 1)
    ctx.fill_noise(s2, px, 2)
    coh, ig, mask, sm = ctx.alloc(px * 4), ctx.alloc(px * 8), ctx.alloc(px), ctx.alloc(K.SUMMARY_BYTES)
    steps = {}
    bufs = [s1, s2, coh, ig, mask, sm]
    for ha, hr in windows:
        cp = sarx.CoherenceParams(window=(ha, hr), threshold=0.5, power_floor=0.1).c_params()
        ws = ctx.alloc(K.workspace_bytes(cp, n, n))
        bufs.append(ws)
        steps[f"coh_{ha}_{hr}"] = (lambda cp=cp: K.enqueue_pair(ctx, s1.ptr, s2.ptr, n, n, cp, coh.ptr), 20)
        steps[f"coh_{ha}_{hr}_igram_mask"] = (lambda cp=cp, ws=ws: K.enqueue_pair(ctx, s1.ptr, s2.ptr, n, n, cp, coh.ptr, ig.ptr, mask.ptr,
                                                                                  sm.ptr, ws.ptr), 29)
    bp = sarx.BalanceParams(block=(256, 256)).c_params(n, n)
    table, bws = ctx.alloc(B.table_bytes(bp, n, n)), ctx.alloc(B.workspace_bytes(bp, n, n))
    steps["balance_estimate"] = (lambda: B.enqueue_estimate(ctx, s1.ptr, s2.ptr, n, n, bp, table.ptr, bws.ptr), 16)
    gp = sarx.GmtiParams()
    gcp = gp.c_params()
    slot = ctx.alloc(gp.slot_bytes())
    steps["gmti_cfar"] = (lambda: sarx._ffi.check(ctx.lib.sarx_gmti_cfar_dev(ctx.h, coh.ptr, n, n, C.byref(gcp), slot.ptr + gmti.HEADER_BYTES,
                                                                             slot.ptr), ctx.h), 4)
    bufs += [table, bws, slot]
    for fn, _ in steps.values():                          # warm-up (code objects); the CFAR then reads a coherence plane
        fn()
    ctx.sync()
    times = {k: [] for k in steps}
    for _ in range(rounds):
        for k, (fn, _) in steps.items():                  # one pair of events at a time: the context has 256 slots, the steps may be many
            ctx.record(0)
            for _ in range(reps):
                fn()
            ctx.record(1)
            ctx.sync()
            times[k].append(ctx.elapsed_ms(0, 1) / reps)
    s = sm.download(np.uint8, (K.SUMMARY_BYTES,)).copy().view(K.SUMMARY_DTYPE)[0]
    res = {"n": n, "last_summary": {"n_tested": int(s["n_tested"]), "n_changed": int(s["n_changed"])}}
    for k, (_, bpp) in steps.items():
        med = float(np.median(times[k]))
        floor = px * bpp / (COPY_TBPS * 1e12) * 1e3
        res[k] = {"ms_median": round(med, 4), "ms_rounds": [round(x, 4) for x in times[k]], "bytes_per_pixel": bpp,
                  "GBps": round(px * bpp / (med * 1e-3) / 1e9, 1), "floor_ms": round(floor, 4), "fraction_of_floor": round(floor / med, 3)}
    for b in bufs:
        b.release()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 16384])
    ap.add_argument("--windows", nargs="+", default=["1,1", "4,4", "16,16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    windows = [tuple(int(x) for x in w.split(",")) for w in a.windows]
    import sarx
    ctx = sarx.default_context()
    out = {"device": ctx.info()["name"], "copy_TBps": COPY_TBPS, "windows": [list(w) for w in windows],
           "launches": [time_launches(ctx, n, windows, a.rounds, a.reps) for n in a.sizes]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
