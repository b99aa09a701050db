#!/usr/bin/env python3
"""OS-CFAR launch timings on the GPU (include/sarx_oscfar.h) beside the CA launch at the same windows, in one process: HIP events,
medians of rounds of repetitions.

    python3 tools/bench_oscfar.py [--rounds 5] [--reps 20] [--cases 8192:2,2:8,8 ...] [--out FILE.json]

A case is n:guard_az,guard_rg:train_az,train_rg.  The default cases are guard (2, 2) with train (8, 8) and (16, 16) at 8192^2 and
16384^2, and the worst case for the ordered statistic, guard (0, 0) / train (8, 8) at 8192^2, where the peak rule removes nothing
and every cell is counted.  The planes are the DPCA magnitude of two device-filled complex noise images (exponential power), so
reports are false alarms at pfa 1e-6 and next to none.  Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))

DEFAULT_CASES = ["8192:2,2:8,8", "8192:2,2:16,16", "16384:2,2:8,8", "16384:2,2:16,16", "8192:0,0:8,8"]


def noise_plane(ctx, n):
    px = n * n
    s1, s2 = ctx.alloc(px * 8), ctx.alloc(px * 8)
    ctx.fill_noise(s1, px, 1)
    ctx.fill_noise(s2, px, 2)
    outs = {k: ctx.alloc(px * 4) for k in ("ati_phase", "slc1_mag", "dpca_mag")}
    ctx.ati_dpca(s1, s2, px, 0.0, outs, want_stats=False)
    ctx.sync()
    for b in (s1, s2, outs["ati_phase"], outs["slc1_mag"]):
        b.release()
    return outs["dpca_mag"]


def time_case(ctx, plane, n, guard, train, rounds, reps):
    import sarx
    from sarx import gmti
    lib, h = ctx.lib, ctx.h
    out = {"n": n, "guard": guard, "train": train}
    for method in ("ca", "os"):
        params = sarx.GmtiParams(guard=guard, train=train, method=method)
        cp = params.c_params()
        slot = ctx.alloc(params.slot_bytes())
        launch = lib.sarx_gmti_cfar_dev if method == "ca" else lib.sarx_gmti_oscfar_dev

        def run():
            sarx._ffi.check(launch(h, plane.ptr, n, n, C.byref(cp), slot.ptr + gmti.HEADER_BYTES, slot.ptr), h)

        run(); ctx.sync()                                 # warm-up (code object)
        ms = []
        for _ in range(rounds):
            ctx.record(0)
            for _ in range(reps):
                run()
            ctx.record(1)
            ctx.sync()
            ms.append(ctx.elapsed_ms(0, 1) / reps)
        count = int(np.frombuffer(bytes(slot.download(np.uint8, (16,))), "<u4")[0])
        slot.release()
        out[method] = {"ms_median": float(np.median(ms)), "ms_rounds": [round(x, 4) for x in ms], "reports": count,
                       "alpha": params.resolved()[5], "rank": params.rank()}
    out["os_over_ca"] = out["os"]["ms_median"] / out["ca"]["ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=DEFAULT_CASES)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    ctx = sarx.default_context()
    cases = []
    for c in a.cases:
        n, g, t = c.split(":")
        cases.append((int(n), tuple(int(x) for x in g.split(",")), tuple(int(x) for x in t.split(","))))
    rows = []
    for n in sorted({c[0] for c in cases}):
        plane = noise_plane(ctx, n)
        rows += [time_case(ctx, plane, n, g, t, a.rounds, a.reps) for m, g, t in cases if m == n]
        plane.release()
    line = json.dumps({"device": ctx.info()["name"], "pfa": 1e-6, "rounds": a.rounds, "reps": a.reps, "cases": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
