#!/usr/bin/env python3
"""Focus-velocity search of the back-projection against one focus call per hypothesis (include/sarx_tdbp_search.h).

The script's own waveform (batch_constants(): 22004 samples, 12000-tap chirp), 2500 pulses, a 128 x 128 chip of 1 m pixels, 33
hypotheses on an along-track line of +-16 m/s; the echo is synthesised on the device and stays there.  In one process, on one plan
and lane, timed with the lane's events after a warm-up, medians of rounds:

    search       one tdbp_search, records only
    search+stack the same with the image stack written
    focus x n    n tdbp_gpu(d_image=...) calls, one per hypothesis (each compresses the pulses and uploads its table again)
    search n=1   one hypothesis: what a search costs before the hypotheses (compression, tables, one image)
    metric       the metric launch alone over a stack of n images

and from those the split of the search: per-hypothesis back-projection = (search - search n=1) / (n - 1), the rest = search n=1
minus one such share.  Prints one JSON line (and writes it to --out).

    python3 tools/bench_tdbp_search.py [--pulses 2500] [--chip 128] [--hyps 33] [--rounds 5] [--reps 3] [--out FILE.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))


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
    return round(float(np.median(t)), 4), [round(x, 4) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pulses", type=int, default=2500)
    ap.add_argument("--chip", type=int, default=128)
    ap.add_argument("--hyps", type=int, default=33)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    from sarx import _ffi, tdbp
    ctx = sarx.default_context()
    k = sarx.batch_constants()
    n_p, nx = a.pulses, a.chip
    swath = float(nx)
    rng = np.random.default_rng(1)
    targets = [{"position": np.array([rng.uniform(-0.3, 0.3) * swath, rng.uniform(-0.3, 0.3) * swath, rng.uniform(0, 10.0)]),
                "rcs": float(rng.uniform(1.0, 50.0))} for _ in range(4)]
    t_vec = (np.arange(n_p) - n_p / 2) / k["PRF"]
    pos, vel = sarx.orbit_arc(t_vec, k)
    d_raw, t0, n_s, v_tgt = sarx.run_physics_spotlight(targets, t_vec, pos, vel, 30.0, 15.0, k["Lambda"] * k["R0"] / swath, consts=k,
                                                       device=True)
    hyps = sarx.tdbp_velocity_line(v_tgt, np.array([1.0, 0.0, 0.0]), 16.0, a.hyps)
    n_h = len(hyps)
    plan = tdbp.cached_plan(ctx, k, n_p, n_s, nx, nx)
    pos, vel, tp = (np.ascontiguousarray(x, dtype=np.float64) for x in (pos, vel, t_vec))
    d_rec, d_stack, d_img = ctx.alloc(32 * n_h), ctx.alloc(16 * n_h * nx * nx), ctx.alloc(16 * nx * nx)
    lib = ctx.lib

    def search(n, stack):
        _ffi.check(lib.sarx_tdbp_search_dev(plan.h, d_raw.ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t0),
                                            hyps.ctypes.data, n, swath, d_stack.ptr if stack else None, d_rec.ptr), ctx.h)

    def focus_each():
        for v in hyps:
            sarx.tdbp_gpu(d_raw, pos, vel, t0, n_s, v, tp, swath, nx, nx, consts=k, d_image=d_img)

    out = {"device": ctx.info()["name"], "pulses": n_p, "num_samples": int(n_s), "chip": [nx, nx], "n_hyp": n_h,
           "pixel_pulse_hypotheses": n_p * nx * nx * n_h}
    out["search_ms"], out["search_ms_rounds"] = _median_ms(ctx, lambda: search(n_h, False), a.rounds, a.reps)
    rec = d_rec.download(np.uint8, (32 * n_h,)).view(importlib.import_module("sarx.tdbp_search").RECORD_DTYPE)
    res = sarx.TdbpSearchResult(hyps, rec, None, "")
    out["best_hypothesis"], out["estimate_offset_mps"] = int(np.argmax(rec["s4"])), round(res.estimate("s4").offset, 4)
    tile = _ffi.C.c_int()
    _ffi.check(lib.sarx_tdbp_search_route(plan.h, _ffi.C.byref(tile)), ctx.h)
    out["route"] = "tile" if tile.value else "exact"
    out["window"] = list(plan.last_window())
    out["search_with_stack_ms"], _ = _median_ms(ctx, lambda: search(n_h, True), a.rounds, a.reps)
    out["focus_each_ms"], out["focus_each_ms_rounds"] = _median_ms(ctx, focus_each, a.rounds, max(a.reps // 3, 1))
    out["focus_window"] = list(plan.last_window())
    out["search_one_ms"], _ = _median_ms(ctx, lambda: search(1, False), a.rounds, a.reps)
    out["metric_alone_ms"], _ = _median_ms(
        ctx, lambda: _ffi.check(lib.sarx_tdbp_search_metric_dev(plan.h, d_stack.ptr, n_h, d_rec.ptr), ctx.h), a.rounds, a.reps)
    per_hyp = (out["search_ms"] - out["search_one_ms"]) / max(n_h - 1, 1)
    out["split_ms"] = {"back_projection_per_hypothesis": round(per_hyp, 4), "back_projection": round(per_hyp * n_h, 4),
                       "compression_tables_metric": round(out["search_ms"] - per_hyp * n_h, 4)}
    out["speedup"] = round(out["focus_each_ms"] / out["search_ms"], 3)
    out["ns_per_pixel_pulse_hypothesis"] = round(out["search_ms"] * 1e6 / out["pixel_pulse_hypotheses"], 6)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    for b in (d_raw, d_rec, d_stack, d_img):
        b.release()


if __name__ == "__main__":
    main()
