#!/usr/bin/env python3
"""Two-channel balance timings on the GPU (include/sarx_balance.h): the estimate (both of its launches) and the apply launch, with
and without the DPCA plane and in place, at 8192^2 and 16384^2, timed with HIP events in rounds.

    python3 tools/bench_balance.py [--sizes 8192 16384] [--rounds 5] [--reps 20] [--block 256 256] [--out FILE.json]

The images are two device-filled complex noise planes.  Each figure comes with the bytes the launch has to move (16 B per pixel for
the estimate and for apply, 28 B per pixel for apply with slc1 and the DPCA plane), the time those bytes take at COPY_TBPS (the best
copy this part reaches, README) and the fraction of that floor the launch achieves.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))

COPY_TBPS = 6.0


def time_launches(ctx, n, rounds, reps, params):
    from sarx import balance as B
    px = n * n
    s1, s2, out = ctx.alloc(px * 8), ctx.alloc(px * 8), ctx.alloc(px * 8)
    dm = ctx.alloc(px * 4)
    ctx.fill_noise(s1, px, 1)
    ctx.fill_noise(s2, px, 2)
    cp = params.c_params(n, n)
    table, ws = ctx.alloc(B.table_bytes(cp, n, n)), ctx.alloc(B.workspace_bytes(cp, n, n))
    steps = {"estimate": (lambda: B.enqueue_estimate(ctx, s1.ptr, s2.ptr, n, n, cp, table.ptr, ws.ptr), 16),
             "apply": (lambda: B.enqueue_apply(ctx, None, s2.ptr, n, n, cp, table.ptr, out.ptr, None), 16),
             "apply_dpca": (lambda: B.enqueue_apply(ctx, s1.ptr, s2.ptr, n, n, cp, table.ptr, out.ptr, dm.ptr), 28),
             "apply_in_place": (lambda: B.enqueue_apply(ctx, None, out.ptr, n, n, cp, table.ptr, out.ptr, None), 16)}
    for fn, _ in steps.values():                          # warm-up (code objects)
        fn()
    ctx.sync()
    times = {k: [] for k in steps}
    for _ in range(rounds):
        for slot, (k, (fn, _)) in enumerate(steps.items()):
            ctx.record(2 * slot)
            for _ in range(reps):
                fn()
            ctx.record(2 * slot + 1)
        ctx.sync()
        for slot, k in enumerate(steps):
            times[k].append(ctx.elapsed_ms(2 * slot, 2 * slot + 1) / reps)
    hdr = table.download(np.uint8, (64,)).view(B.HEADER_DTYPE)[0]
    res = {"n": n, "blocks": [int(hdr["nb_az"]), int(hdr["nb_rg"])], "n_valid": int(hdr["n_valid"])}
    for k, (_, bpp) in steps.items():
        med = float(np.median(times[k]))
        floor = px * bpp / (COPY_TBPS * 1e12) * 1e3
        res[k] = {"ms_median": round(med, 4), "ms_rounds": [round(x, 4) for x in times[k]], "bytes_per_pixel": bpp,
                  "GBps": round(px * bpp / (med * 1e-3) / 1e9, 1), "floor_ms": round(floor, 4), "fraction_of_floor": round(floor / med, 3)}
    for b in (s1, s2, out, dm, table, ws):
        b.release()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 16384])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--block", type=int, nargs=2, default=[256, 256])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    ctx = sarx.default_context()
    params = sarx.BalanceParams(block=tuple(a.block))
    out = {"device": ctx.info()["name"], "copy_TBps": COPY_TBPS,
           "params": {"block": list(params.block), "mode": params.mode, "interp": params.interp},
           "launches": [time_launches(ctx, n, a.rounds, a.reps, params) for n in a.sizes]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
