#!/usr/bin/env python3
"""GMTI refocus timings on the GPU (include/sarx_refocus.h): one sarx_refocus_dev call (the curve and record launches) on 8192^2
device images for 64, 1024 and 4096 reports, chip (256, 5) and 33 hypotheses by default, timed with HIP events in rounds.  The
split between the two launches comes from a rocprofv3 kernel trace of the same script.

    python3 tools/bench_refocus.py [--n 8192] [--reports 64 1024 4096] [--chip 256 5] [--n-hyp 33] [--rounds 5] [--reps 20]
                                   [--out FILE.json]

The images are device-filled complex noise, the reports uniformly placed cells of a slot uploaded once (the detector's output
format; the header holds the count).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))


def time_call(ctx, s1, s2, n, n_rep, params, rounds, reps):
    import sarx
    from sarx import refocus
    rng = np.random.default_rng(n_rep)
    pos = np.stack([rng.integers(0, n, n_rep), rng.integers(0, n, n_rep)], axis=1)
    raw, _ = refocus.positions_slot(pos, n, n)
    slot = ctx.to_device(raw)
    rec = ctx.alloc(params.record_bytes(n_rep))
    k = sarx.radar.reference_constants()
    cp = params.c_params(k["Lambda"], k["V_eff"], k["PRF"], k["R0"], k["C"] / (2 * k["FS"]), 0.0)

    def call():
        refocus.enqueue(ctx, s1.ptr, s2.ptr, n, n, cp, slot.ptr, n_rep, rec.ptr)

    call(); ctx.sync()                                    # warm-up (code objects, the curve scratch buffer)
    ms = []
    for _ in range(rounds):
        ctx.record(0)
        for _ in range(reps):
            call()
        ctx.record(1)
        ctx.sync()
        ms.append(ctx.elapsed_ms(0, 1) / reps)
    out = rec.download(np.uint8, (params.record_bytes(n_rep),)).view(refocus.RECORD_DTYPE)
    assert (out["i0"] >= 0).all()
    for b in (slot, rec):
        b.release()
    med = float(np.median(ms))
    return {"reports": n_rep, "ms_median": med, "ms_rounds": [round(x, 4) for x in ms], "us_per_report": med * 1e3 / n_rep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--reports", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--chip", type=int, nargs=2, default=[256, 5])
    ap.add_argument("--n-hyp", type=int, default=33)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    import sarx.radar  # noqa: F401
    ctx = sarx.default_context()
    px = a.n * a.n
    s1, s2 = ctx.alloc(px * 8), ctx.alloc(px * 8)
    ctx.fill_noise(s1, px, 1)
    ctx.fill_noise(s2, px, 2)
    params = sarx.RefocusParams(chip=tuple(a.chip), n_hyp=a.n_hyp)
    out = {"device": ctx.info()["name"], "n": a.n, "chip": a.chip, "n_hyp": a.n_hyp,
           "calls": [time_call(ctx, s1, s2, a.n, r, params, a.rounds, a.reps) for r in a.reports]}
    s1.release()
    s2.release()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
