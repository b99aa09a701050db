#!/usr/bin/env python3
"""GMTI detector timings on the GPU (include/sarx_gmti.h): the CFAR and refine launches at 8192^2 and 16384^2, timed with HIP events
in rounds, and TwoChannelBatch(stack="detections") frames/s at 8192^2 against stack="products" (same frames, same process).

    python3 tools/bench_gmti.py [--sizes 8192 16384] [--rounds 5] [--reps 20] [--frames 8] [--out FILE.json]

The planes are the DPCA magnitude of two device-filled complex noise images (exponential power: the CFAR's design clutter), so
detections are the false alarms at the chosen pfa.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))


def time_launches(ctx, n, rounds, reps, params):
    import sarx
    from sarx import gmti
    px = n * n
    s1, s2 = ctx.alloc(px * 8), ctx.alloc(px * 8)
    ctx.fill_noise(s1, px, 1)
    ctx.fill_noise(s2, px, 2)
    outs = {k: ctx.alloc(px * 4) for k in ("ati_phase", "slc1_mag", "dpca_mag")}
    ctx.ati_dpca(s1, s2, px, 0.0, outs, want_stats=False)
    slot = ctx.alloc(params.slot_bytes())
    cp = params.c_params()
    import ctypes as C
    lib, h = ctx.lib, ctx.h
    rep_ptr = slot.ptr + gmti.HEADER_BYTES

    def cfar():
        sarx._ffi.check(lib.sarx_gmti_cfar_dev(h, outs["dpca_mag"].ptr, n, n, C.byref(cp), rep_ptr, slot.ptr), h)

    def refine():
        sarx._ffi.check(lib.sarx_gmti_refine_dev(h, s1.ptr, s2.ptr, n, n, 0.0, rep_ptr, slot.ptr, cp.max_detections), h)

    cfar(); refine(); ctx.sync()                          # warm-up (code objects, the refine copy buffer)
    res = {"cfar_ms": [], "refine_ms": []}
    for _ in range(rounds):
        ctx.record(0)
        for _ in range(reps):
            cfar()
        ctx.record(1)
        for _ in range(reps):
            refine()
        ctx.record(2)
        ctx.sync()
        res["cfar_ms"].append(ctx.elapsed_ms(0, 1) / reps)
        res["refine_ms"].append(ctx.elapsed_ms(1, 2) / reps)
    count = int(np.frombuffer(bytes(slot.download(np.uint8, (16,))), "<u4")[0])
    for b in (s1, s2, slot, *outs.values()):
        b.release()
    return {"n": n, "cfar_ms_median": float(np.median(res["cfar_ms"])), "refine_ms_median": float(np.median(res["refine_ms"])),
            "cfar_ms_rounds": [round(x, 4) for x in res["cfar_ms"]], "refine_ms_rounds": [round(x, 4) for x in res["refine_ms"]],
            "reports": count, "plane_read_GBps": px * 4 / (float(np.median(res["cfar_ms"])) * 1e-3) / 1e9}


def batch_fps(ctx, n, frames, stack, params):
    from sarx.batch import TwoChannelBatch
    b = TwoChannelBatch(ctx, n, frames, stack=stack, detect=params if stack == "detections" else None)
    b.prepare()
    b.run(); ctx.sync()                                   # warm-up
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        b.run()
        ctx.sync()
        times.append(time.perf_counter() - t0)
    slot = b.slot_bytes
    b.close()
    return {"stack": stack, "frames_per_s": frames / float(np.median(times)), "slot_bytes": slot,
            "run_s": [round(t, 4) for t in times]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 16384])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--batch-n", type=int, default=8192)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    ctx = sarx.default_context()
    params = sarx.GmtiParams()
    out = {"device": ctx.info()["name"], "params": {"guard": params.guard, "train": params.train, "pfa": params.pfa,
                                                  "max_detections": params.max_detections},
           "launches": [time_launches(ctx, n, a.rounds, a.reps, params) for n in a.sizes]}
    if a.frames > 0:
        out["batch"] = [batch_fps(ctx, a.batch_n, a.frames, s, params) for s in ("products", "detections")]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
