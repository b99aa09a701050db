#!/usr/bin/env python3
"""One step of the Kalman ground tracker (include/sarx_ktrack.h) for 16, 1024 and 16384 reports against as many
live tracks, beside one step of the existing tracker (include/sarx_track.h) at the same counts, from the same tree.

Movers on a square lattice 150 m apart seen from 30 km away at 10 km height; the first step gives every report a track, every later
step (the same frame again: dt = 0) matches every track with its report, so each timed step runs the prediction, both searches, n
Kalman updates and the resolve launch with no birth.  The coarse box of 60 m holds one report per track: a sparse scene, where
the staged searches reject nearly every pair at the first comparison.  The existing tracker steps over the same lattice in pixels
(20 apart, gate 4).  One process, one lane, timed with the lane's events after a warm-up: the median over --rounds of --reps
back-to-back steps.  Prints one JSON line (and writes it to --out).

    python3 tools/bench_ktrack.py [--rounds 9] [--reps 50] [--out FILE]"""
import argparse
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
    from sarx import ktrack, relocate, slot, track
    ctx = sarx.default_context()
    info = ctx.info()
    rng = np.random.default_rng(5)
    pos_ref, vel_ref = (30000.0, 0.0, 10000.0), (0.0, 218.0, 0.0)
    out = {"device": info["name"] or info["arch"], "arch": info["arch"], "rounds": a.rounds, "reps": a.reps, "rows": []}
    for n in (16, 1024, 16384):
        side = int(np.ceil(np.sqrt(n)))
        k = np.arange(n)
        rep = np.zeros(n, slot.REPORT_DTYPE)
        rep["i"], rep["j"] = 20 * (k // side), 20 * (k % side)
        rep["power"], rep["mean"] = rng.uniform(20, 40, n), 1.0
        rec = np.zeros(n, relocate.RECORD_DTYPE)
        rec["x"], rec["y"] = 150.0 * (k % side - side / 2.0) + rng.uniform(-1, 1, n), 150.0 * (k // side - side / 2.0) + rng.uniform(-1, 1, n)
        rec["rank"] = -1
        kp = sarx.KalmanTrackParams(gate_m=60.0, max_tracks=n, max_detections=n)
        tp = sarx.TrackParams(max_tracks=n, max_detections=n)
        kcp, tcp = kp.c_params(), tp.c_params()
        frame = ktrack.c_frame(0.0, pos_ref, vel_ref, 0)
        bufs = [ctx.to_device(slot.encode(rep, n)), ctx.to_device(rec), ctx.to_device(rng.uniform(-9, 9, n)),
                ctx.alloc(ktrack.table_bytes(kcp)), ctx.alloc(ktrack.workspace_bytes(kcp)), ctx.alloc(4 * n),
                ctx.alloc(track.table_bytes(tcp)), ctx.alloc(track.workspace_bytes(tcp))]
        d_slot, d_rec, d_v, k_table, k_ws, d_assoc, t_table, t_ws = bufs

        def kalman():
            ktrack.enqueue_step(ctx, kcp, frame, d_slot.ptr, d_rec.ptr, (d_v.ptr, 8), k_table.ptr, d_assoc.ptr, k_ws.ptr)

        def existing():
            track.enqueue_step(ctx, tcp, d_slot.ptr, 0, t_table.ptr, d_assoc.ptr, t_ws.ptr)

        ktrack.enqueue_init(ctx, kcp, k_table.ptr)
        track.enqueue_init(ctx, tcp, t_table.ptr)
        k_us = _median_us(ctx, kalman, a.rounds, a.reps)
        t_us = _median_us(ctx, existing, a.rounds, a.reps)
        kh = k_table.download(np.uint8, (64,)).view(ktrack.HEADER_DTYPE)[0]
        th = t_table.download(np.uint8, (64,)).view(track.HEADER_DTYPE)[0]
        assert int(kh["error"]) == 0 and int(th["error"]) == 0 and int(kh["n_live"]) == n == int(th["n_live"]), (kh, th)
        matched = int(np.count_nonzero(d_assoc.download(np.int32, (n,)) >= 0))
        out["rows"].append({"reports": n, "tracks": n, "matched": matched, "ktrack_step_us": k_us[0], "ktrack_min": k_us[1], "ktrack_max": k_us[2],
                            "track_step_us": t_us[0], "track_min": t_us[1], "track_max": t_us[2]})
        for b in bufs:
            b.release()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
