#!/usr/bin/env python3
"""The ground relocation's two launches (include/sarx_relocate.h) for 16, 1024 and 16384 reports.

Reports spread over a 512 x 512 image of 2 m pixels seen from a 5 km circle at 3 km height, seeded speeds within +-9 m/s, every
report kept on a 1024 x 1024 output grid of 2 m (so the slot launch ranks and copies all of them: its worst case).  One process,
one lane, timed with the lane's events after a warm-up: the median over --rounds of --reps back-to-back sarx_relocate_dev calls.
Prints one JSON line (and writes it to --out).

    python3 tools/bench_relocate.py [--rounds 9] [--reps 50] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))


def _median_us(ctx, fn, rounds, reps):
    for _ in range(3):
        fn()
    ctx.sync()
    t = []
    for _ in range(rounds):
        ctx.record(0)
        for _ in range(reps):
            fn()
        ctx.record(1)
        ctx.sync()
        t.append(1e3 * ctx.elapsed_ms(0, 1) / reps)
    return round(float(np.median(t)), 2), round(float(np.min(t)), 2), round(float(np.max(t)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    from sarx import _ffi, relocate, slot
    ctx = sarx.default_context()
    info = ctx.info()
    rng = np.random.default_rng(5)
    pos_ref, vel_ref = (5000.0 * np.cos(0.4), 5000.0 * np.sin(0.4), 3000.0), (-150.0 * np.sin(0.4), 150.0 * np.cos(0.4), 0.0)
    out = {"device": info["name"] or info["arch"], "arch": info["arch"], "rounds": a.rounds, "reps": a.reps, "rows": []}
    for n in (16, 1024, 16384):
        rep = np.zeros(n, slot.REPORT_DTYPE)
        rep["i"], rep["j"] = rng.integers(0, 512, n), rng.integers(0, 512, n)
        rep["power"], rep["mean"] = rng.uniform(20, 40, n), 1.0
        prm = relocate.relocate_params(pos_ref, vel_ref, (1022.0, 512, 512), (-1024.0, -1024.0, 2.0, 2.0, 1024, 1024), n)
        bufs = [ctx.to_device(slot.encode(rep, n)), ctx.to_device(rng.uniform(-9, 9, n)), ctx.to_device(rng.uniform(-9, 9, n)),
                ctx.alloc(64 * n), ctx.alloc(slot.slot_bytes(n))]
        d_slot, d_v, d_along, d_rec, d_out = bufs

        def run():
            _ffi.check(ctx.lib.sarx_relocate_dev(ctx.h, C.byref(prm), d_slot.ptr, d_v.ptr, 8, None, 0, d_along.ptr, 8, d_rec.ptr, d_out.ptr), ctx.h)

        med, lo, hi = _median_us(ctx, run, a.rounds, a.reps)
        kept = slot.header(slot.fetch_header(ctx, d_out.ptr))[0]
        out["rows"].append({"reports": n, "kept": kept, "us": med, "us_min": lo, "us_max": hi})
        for b in bufs:
            b.release()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
