#!/usr/bin/env python3
"""GMTI ATI gate timings on the GPU (include/sarx_atigate.h): one sarx_atigate_step_dev (both launches) at 64, 1024 and 4096
reports on 8192^2 clutter-plus-noise planes (common clutter, independent noise 10 dB below it in each channel: coherence 0.91), with
the windows (2, 2) / (8, 8) / (1, 1) and (4, 2) / (28, 30) / (4, 2) - the 32-wide one - and, in the same process and on the same
planes and report lists, the refine launch and the refocus (default RefocusParams) the stage stands beside.  HIP events, medians of
rounds.

    python3 tools/bench_atigate.py [--n 8192] [--rounds 5] [--reps 20] [--out FILE.json]

The slots have a capacity of 4096 reports.  Beside each time: the bytes a report reads (outer box x two images x 8 bytes, clipped
boxes counted whole) and the step's share of refine + refocus at the same report count.  Prints one JSON line (and writes it to
--out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))
WINDOWS = {"default": ((2, 2), (8, 8), (1, 1)), "wide": ((4, 2), (28, 30), (4, 2))}
CAPACITY = 4096


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


def planes(ctx, n):
    """a = c + n1, b = c + n2 on the device: c complex noise, n1 and n2 independent thermal noise 10 dB below it."""
    from sarx import noise
    px = n * n
    a, b = ctx.alloc(px * 8), ctx.alloc(px * 8)
    ctx.fill_noise(a, px, 11)
    import sarx
    sarx._ffi.check(ctx.lib.sarx_memcpy_d2d(ctx.h, b.ptr, a.ptr, px * 8), ctx.h)
    _, mean = noise.power_stats(a, px, ctx)
    noise.add_noise_dev(a, px, mean, 10.0, scr_db=None, seed=12, ctx=ctx)
    noise.add_noise_dev(b, px, mean, 10.0, scr_db=None, seed=13, ctx=ctx)
    return a, b


def reports(n_img, count, seed=1):
    from sarx import gmti
    flat = np.sort(np.random.default_rng(seed).choice(n_img * n_img, count, replace=False))      # sorted by (i, j), no cell twice
    rep = np.zeros(count, gmti.REPORT_DTYPE)
    rep["i"], rep["j"] = flat // n_img, flat % n_img
    rep["power"], rep["mean"] = 30.0, 1.0
    return rep


def time_case(ctx, a, b, n_img, count, rounds, reps):
    import sarx
    from sarx import atigate as K, refocus as R, track
    rep = reports(n_img, count)
    raw = track.encode_slot(rep, CAPACITY)
    d_in, d_out = ctx.to_device(raw), ctx.alloc(raw.size)
    out = {"reports": count, "capacity": CAPACITY}
    for name, (guard, train, looks) in WINDOWS.items():
        cp = sarx.AtiGateParams(guard=guard, train=train, looks=looks).c_params(CAPACITY)
        d_stats = ctx.alloc(K.stats_bytes(cp))
        med, per = _median_ms(ctx, lambda: K.enqueue_step(ctx, cp, a.ptr, b.ptr, n_img, n_img, d_in.ptr, d_out.ptr, d_stats.ptr), rounds, reps)
        st = d_stats.download(np.uint8, (96 * count,)).view(K.GATE_DTYPE)
        cells = (2 * (guard[0] + train[0]) + 1) * (2 * (guard[1] + train[1]) + 1)
        out[name] = {"step_ms_median": med, "step_ms_rounds": per, "bytes_read_per_report": cells * 2 * 8,
                     "kept": int(d_out.download(np.uint32, (4,))[0]), "passed": int((st["status"] == K.PASSED).sum()),
                     "rejected": int((st["status"] == K.REJECTED).sum()), "untested": int((st["status"] == K.UNTESTED).sum())}
        d_stats.release()
    # the stages it stands beside, on the same list: refine (sorts the list and sums the 3 x 3 interferograms) and refocus
    lib, h = ctx.lib, ctx.h
    refine = lambda: sarx._ffi.check(lib.sarx_gmti_refine_dev(h, a.ptr, b.ptr, n_img, n_img, 0.0, d_in.ptr + 16, d_in.ptr, CAPACITY), h)
    out["refine_ms_median"], out["refine_ms_rounds"] = _median_ms(ctx, refine, rounds, reps)
    rp = sarx.RefocusParams()
    rcp = rp.c_params(0.03, 200.0, 1000.0, 10000.0, 1.5, 0.0)
    d_rec = ctx.alloc(rp.record_bytes(CAPACITY))
    out["refocus_ms_median"], out["refocus_ms_rounds"] = _median_ms(
        ctx, lambda: R.enqueue(ctx, a.ptr, b.ptr, n_img, n_img, rcp, d_in.ptr, CAPACITY, d_rec.ptr), rounds, max(reps // 4, 1))
    beside = out["refine_ms_median"] + out["refocus_ms_median"]
    for name in WINDOWS:
        out[name]["share_of_refine_plus_refocus"] = round(out[name]["step_ms_median"] / beside, 4)
    for x in (d_in, d_out, d_rec):
        x.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sarx
    ctx = sarx.default_context()
    a, b = planes(ctx, args.n)
    out = {"device": ctx.info()["name"], "n": args.n, "windows": {k: [list(x) for x in v] for k, v in WINDOWS.items()},
           "cases": [time_case(ctx, a, b, args.n, count, args.rounds, args.reps) for count in (64, 1024, 4096)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
