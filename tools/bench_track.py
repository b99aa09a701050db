#!/usr/bin/env python3
"""GMTI tracker timings on the GPU (include/sarx_track.h): one step (both launches) at (live tracks, reports) = (64, 64),
(1024, 1024) and (4096, 4096), each of its two launches alone, a 64-frame sarx_track_run_dev, the CFAR's per-frame time at 8192^2 in
the same process as the yardstick, and batch frames/s for stack="detections" at 8192^2 with 8 frames with and without track=.
HIP events, medians of rounds.

    python3 tools/bench_track.py [--rounds 5] [--reps 20] [--no-batch] [--out FILE.json]

A step is timed in its steady state: the table holds k confirmed tracks at rest and the slot reports the same k pixels, so every
step matches all k and the table stays as it is (k x k pairs go through the gate pre-test, k through the divisions).  The table has
the capacity the case needs (k slots, k reports).  Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))


def _grid_slot(k, max_det, seed=1):
    """k reports on a 12-pixel grid (gates 4 x 4 do not touch), sorted by (i, j), as one slot's bytes."""
    from sarx import gmti, track
    side = int(np.ceil(np.sqrt(k)))
    idx = np.arange(k)
    rep = np.zeros(k, gmti.REPORT_DTYPE)
    rep["i"], rep["j"] = 12 * (idx // side) + 8, 12 * (idx % side) + 8
    rng = np.random.default_rng(seed)
    rep["mean"], rep["power"] = 1.0, 30.0 + rng.random(k)
    rep["interf_re"], rep["interf_im"] = rep["power"], 0.0
    return track.encode_slot(rep, max_det)


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


def time_step(ctx, k, rounds, reps):
    import sarx
    from sarx import track as T
    tp = sarx.TrackParams(max_tracks=k, max_detections=k)
    cp = tp.c_params()
    slot = ctx.to_device(_grid_slot(k, k))
    table, ws, row = ctx.alloc(T.table_bytes(cp)), ctx.alloc(T.workspace_bytes(cp)), ctx.alloc(k * 4)
    T.enqueue_init(ctx, cp, table.ptr)
    for f in range(6):                                     # births, then confirmed and at rest
        T.enqueue_step(ctx, cp, slot.ptr, f, table.ptr, row.ptr, ws.ptr)
    hdr = table.download(np.uint8, (64,)).view(T.HEADER_DTYPE)[0]
    assert hdr["n_live"] == k and hdr["n_confirmed"] == k and hdr["error"] == 0, hdr
    med, per = _median_ms(ctx, lambda: T.enqueue_step(ctx, cp, slot.ptr, 6, table.ptr, row.ptr, ws.ptr), rounds, reps)
    hdr = table.download(np.uint8, (64,)).view(T.HEADER_DTYPE)[0]
    assert hdr["n_live"] == k and hdr["error"] == 0
    for b in (slot, table, ws, row):
        b.release()
    return {"live_tracks": k, "reports": k, "step_ms_median": med, "step_ms_rounds": per}


def time_run(ctx, n_frames, k, rounds, reps):
    import sarx
    from sarx import track as T
    tp = sarx.TrackParams(max_tracks=k, max_detections=k)
    cp = tp.c_params()
    one = _grid_slot(k, k)
    stack = ctx.to_device(np.tile(one, (n_frames, 1)))
    table, ws, assoc = ctx.alloc(T.table_bytes(cp)), ctx.alloc(T.workspace_bytes(cp)), ctx.alloc(n_frames * k * 4)

    def run():
        T.enqueue_init(ctx, cp, table.ptr)
        T.enqueue_run(ctx, cp, stack.ptr, one.size, n_frames, table.ptr, assoc.ptr, ws.ptr)
    med, per = _median_ms(ctx, run, rounds, max(reps // 4, 1))
    for b in (stack, table, ws, assoc):
        b.release()
    return {"frames": n_frames, "live_tracks": k, "reports": k, "run_ms_median": med, "run_ms_rounds": per,
            "ms_per_frame": round(med / n_frames, 5)}


def time_cfar(ctx, n, rounds, reps):
    """The detector's CFAR launch on an [n x n] noise magnitude plane: the per-frame cost the tracker's step stands beside."""
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


def time_batch(ctx, n, frames, rounds):
    """frames/s of TwoChannelBatch(stack="detections") on noise frames, with and without track=, alternating."""
    import sarx
    from sarx.batch import TwoChannelBatch
    det = sarx.GmtiParams()
    out = {"n": n, "frames": frames}
    rates = {"without_track": [], "with_track": []}
    batches = {"without_track": TwoChannelBatch(ctx, n, frames, stack="detections", detect=det),
               "with_track": TwoChannelBatch(ctx, n, frames, stack="detections", detect=det, track=sarx.TrackParams(max_tracks=16384))}
    for b in batches.values():
        b.run()
        ctx.sync()
    for _ in range(rounds):
        for k, b in batches.items():
            t0 = time.perf_counter()
            b.run()
            ctx.sync()
            rates[k].append(frames / (time.perf_counter() - t0))
    for k, b in batches.items():
        out[k] = {"frames_per_s_median": round(float(np.median(rates[k])), 2), "frames_per_s_rounds": [round(x, 2) for x in rates[k]]}
        b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-batch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    ctx = sarx.default_context()
    out = {"device": ctx.info()["name"],
           "steps": [time_step(ctx, k, a.rounds, a.reps) for k in (64, 1024, 4096)],
           "run": time_run(ctx, 64, 1024, a.rounds, a.reps),
           "cfar": time_cfar(ctx, 8192, a.rounds, a.reps)}
    if not a.no_batch:
        out["batch"] = time_batch(ctx, 8192, 8, a.rounds)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
