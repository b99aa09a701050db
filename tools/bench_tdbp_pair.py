#!/usr/bin/env python3
"""Two-receiver back-projection against two single-channel focus calls (include/sarx_tdbp_pair.h).

The script's own waveform (batch_constants(): 22004 samples, 12000-tap chirp), 2500 pulses, two channels resident on the device
(two spotlight echoes synthesised there: the time of a launch does not depend on what the samples hold), chips of 128 x 128 and
512 x 512 pixels of 1 m.  In one process, on one plan and lane, timed with the lane's events after a warm-up, medians of rounds:

    pair c64     one sarx_tdbp_pair_dev with the DPCA pulse shift, complex64 pair written
    pair c128    the same, complex128 pair written
    focus x 2    two tdbp_gpu(d_image=...) calls on the same lane: the yardstick.  They do somewhat different arithmetic (the
                 stop-and-go receiver and the Doppler time shift of the spotlight generator, and the tile-expanded geometry where
                 its condition holds; the pair has neither and runs the exact form only).

Prints one JSON line (and writes it to --out).

    python3 tools/bench_tdbp_pair.py [--pulses 2500] [--chips 128,512] [--rounds 5] [--reps 3] [--out FILE.json]"""
import argparse
import ctypes as C
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
    ap.add_argument("--chips", default="128,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    from sarx import _ffi, tdbp
    from sarx.tdbp_pair import pair_params
    ctx = sarx.default_context()
    k = sarx.batch_constants()
    n_p = a.pulses
    rng = np.random.default_rng(1)
    targets = [{"position": np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), 0.0]), "rcs": float(rng.uniform(1.0, 50.0))} for _ in range(4)]
    t_vec = (np.arange(n_p) - n_p / 2) / k["PRF"]
    pos, vel = sarx.orbit_arc(t_vec, k)
    raws = []
    for _ in range(2):
        d_raw, t0, n_s, _ = sarx.run_physics_spotlight(targets, t_vec, pos, vel, 30.0, 0.0, k["Lambda"] * k["R0"] / 128.0, consts=k, device=True)
        raws.append(d_raw)
    pos, vel, tp = (np.ascontiguousarray(x, dtype=np.float64) for x in (pos, vel, t_vec))
    speed = float(np.linalg.norm(vel[n_p // 2]))
    prm = pair_params(n_p, (-speed / k["PRF"], speed / k["PRF"]), 0.0, True)
    vf = np.zeros(3)
    out = {"device": ctx.info()["name"], "pulses": n_p, "num_samples": int(n_s), "chips": []}
    for nx in (int(c) for c in a.chips.split(",")):
        swath = float(nx)
        plan = tdbp.cached_plan(ctx, k, n_p, n_s, nx, nx)
        d128, d64, d_img = ctx.alloc(32 * nx * nx), ctx.alloc(16 * nx * nx), ctx.alloc(16 * nx * nx)

        def pair(wide):
            _ffi.check(ctx.lib.sarx_tdbp_pair_dev(plan.h, raws[0].ptr, raws[1].ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t0),
                                                  vf.ctypes.data, swath, C.byref(prm), d128.ptr if wide else None, None if wide else d64.ptr), ctx.h)

        def focus_two():
            for r in raws:
                sarx.tdbp_gpu(r, pos, vel, t0, n_s, vf, tp, swath, nx, nx, consts=k, d_image=d_img)

        row = {"chip": [nx, nx], "pixel_pulses_per_channel": n_p * nx * nx}
        row["pair_c64_ms"], row["pair_c64_ms_rounds"] = _median_ms(ctx, lambda: pair(False), a.rounds, a.reps)
        row["pair_window"] = list(plan.last_window())
        tile = C.c_int()
        _ffi.check(ctx.lib.sarx_tdbp_pair_route(plan.h, C.byref(tile)), ctx.h)
        row["pair_route"] = "tile" if tile.value else "exact"
        row["pair_c128_ms"], _ = _median_ms(ctx, lambda: pair(True), a.rounds, a.reps)
        row["focus_two_ms"], row["focus_two_ms_rounds"] = _median_ms(ctx, focus_two, a.rounds, a.reps)
        row["focus_window"] = list(plan.last_window())
        row["pair_over_two_focus"] = round(row["pair_c64_ms"] / row["focus_two_ms"], 3)
        row["pair_ns_per_pixel_pulse_channel"] = round(row["pair_c64_ms"] * 1e6 / (2 * n_p * nx * nx), 6)
        out["chips"].append(row)
        for b in (d128, d64, d_img):
            b.release()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    for b in raws:
        b.release()


if __name__ == "__main__":
    main()
