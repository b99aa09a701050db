#!/usr/bin/env python3
"""N-receiver back-projection against the same channels through the calls that existed before it, and the resolver
(include/sarx_tdbp_multi.h).

The script's own waveform (batch_constants(): 22004 samples, 12000-tap chirp), 2500 pulses, four channels resident on the device
(spotlight echoes synthesised there: the time of a launch does not depend on what the samples hold), a chip of 512 x 512 pixels.
In one process, on one plan and lane, timed with the lane's events after a warm-up, in the order A B B A per channel count:

    A  multi    one sarx_tdbp_multi_dev with n_rx = 3 or 4, complex64 stack written
    B  parts    one sarx_tdbp_pair_dev (channels 0, 1) plus n_rx - 2 tdbp_gpu(d_image=...) calls on the same lane: the yardstick.
                The focus calls do somewhat different arithmetic (the stop-and-go receiver and the Doppler time shift of the
                spotlight generator), and each call picks its own route: `routes` tells which ran.

and the resolver's launch for 16 and for 1024 reports spread over the chip.  Prints one JSON line (and writes it to --out).

    python3 tools/bench_tdbp_multi.py [--pulses 2500] [--chip 512] [--pixel 1.0] [--offsets -1,1,9,6.3] [--rounds 5] [--reps 3] [--out FILE]"""
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
    return round(float(np.median(t)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pulses", type=int, default=2500)
    ap.add_argument("--chip", type=int, default=512)
    ap.add_argument("--pixel", type=float, default=1.0, help="pixel size in metres (the tile route needs small ones for a long baseline)")
    ap.add_argument("--offsets", default="-1,1,9,6.3", help="receiver offsets in units of V / PRF")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    from sarx import _ffi, slot, tdbp
    from sarx.tdbp_multi import RECORD_DTYPE, multi_params, resolve_params
    from sarx.tdbp_pair import pair_params
    ctx = sarx.default_context()
    k = sarx.batch_constants()
    n_p, nx = a.pulses, a.chip
    rng = np.random.default_rng(1)
    targets = [{"position": np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), 0.0]), "rcs": float(rng.uniform(1.0, 50.0))} for _ in range(4)]
    t_vec = (np.arange(n_p) - n_p / 2) / k["PRF"]
    pos, vel = sarx.orbit_arc(t_vec, k)
    raws = []
    for _ in range(4):
        d_raw, t0, n_s, _ = sarx.run_physics_spotlight(targets, t_vec, pos, vel, 30.0, 0.0, k["Lambda"] * k["R0"] / 128.0, consts=k, device=True)
        raws.append(d_raw)
    pos, vel, tp = (np.ascontiguousarray(x, dtype=np.float64) for x in (pos, vel, t_vec))
    speed = float(np.linalg.norm(vel[n_p // 2]))
    offs = [float(x) * speed / k["PRF"] for x in a.offsets.split(",")]
    vf = np.zeros(3)
    swath = nx * a.pixel
    plan = tdbp.cached_plan(ctx, k, n_p, n_s, nx, nx)
    d_stack, d_img = ctx.alloc(4 * 8 * nx * nx), ctx.alloc(16 * nx * nx)
    info = ctx.info()
    out = {"device": info["name"] or info["arch"], "arch": info["arch"], "compute_units": info["compute_units"], "pulses": n_p, "num_samples": int(n_s), "chip": [nx, nx], "pixel_m": a.pixel,
           "offsets_in_pulses": a.offsets, "rows": []}
    pair_prm = pair_params(n_p, offs[:2], 0.0, False)
    for n_rx in (3, 4):
        prm = multi_params(n_p, offs[:n_rx], 0.0, ((0,) * n_rx, n_p))
        ptrs = (C.c_void_p * n_rx)(*(r.ptr for r in raws[:n_rx]))

        def multi():
            _ffi.check(ctx.lib.sarx_tdbp_multi_dev(plan.h, ptrs, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t0), vf.ctypes.data,
                                                   swath, C.byref(prm), None, d_stack.ptr), ctx.h)

        def parts():
            _ffi.check(ctx.lib.sarx_tdbp_pair_dev(plan.h, raws[0].ptr, raws[1].ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t0),
                                                  vf.ctypes.data, swath, C.byref(pair_prm), None, d_stack.ptr), ctx.h)
            for r in raws[2:n_rx]:
                sarx.tdbp_gpu(r, pos, vel, t0, n_s, vf, tp, swath, nx, nx, consts=k, d_image=d_img)

        row = {"n_rx": n_rx, "pixel_pulses_per_channel": n_p * nx * nx}
        order = [("multi", multi), ("parts", parts), ("parts", parts), ("multi", multi)]
        times = {"multi": [], "parts": []}
        for name, fn in order:
            times[name].append(_median_ms(ctx, fn, a.rounds, a.reps))
        tile, ptile = C.c_int(), C.c_int()
        _ffi.check(ctx.lib.sarx_tdbp_multi_route(plan.h, C.byref(tile)), ctx.h)
        _ffi.check(ctx.lib.sarx_tdbp_pair_route(plan.h, C.byref(ptile)), ctx.h)
        row["routes"] = {"multi": "tile" if tile.value else "exact", "pair": "tile" if ptile.value else "exact"}
        row["multi_ms_abba"], row["parts_ms_abba"] = times["multi"], times["parts"]
        row["multi_ms"], row["parts_ms"] = round(float(np.mean(times["multi"])), 4), round(float(np.mean(times["parts"])), 4)
        row["multi_over_parts"] = round(row["multi_ms"] / row["parts_ms"], 3)
        row["multi_ns_per_pixel_pulse_channel"] = round(row["multi_ms"] * 1e6 / (n_rx * n_p * nx * nx), 6)
        out["rows"].append(row)
    # the resolver on the four-channel stack that the last multi call left
    lags = [(o - offs[0]) / (2 * speed) for o in offs[1:]]
    out["resolve"] = []
    for n_rep in (16, 1024):
        rep = np.zeros(n_rep, slot.REPORT_DTYPE)
        rep["i"], rep["j"] = rng.integers(0, nx, n_rep), rng.integers(0, nx, n_rep)
        d_slot = ctx.to_device(slot.encode(rep, n_rep))
        d_rec = ctx.alloc(n_rep * RECORD_DTYPE.itemsize)
        rp = resolve_params(lags, k["Lambda"], 30.0, 1, n_rep)

        def resolve():
            _ffi.check(ctx.lib.sarx_tdbp_multi_resolve_dev(ctx.h, C.byref(rp), d_stack.ptr, nx, nx, d_slot.ptr, d_rec.ptr), ctx.h)

        out["resolve"].append({"reports": n_rep, "ms": _median_ms(ctx, resolve, a.rounds, 10)})
        d_slot.release()
        d_rec.release()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    for b in (d_stack, d_img, *raws):
        b.release()


if __name__ == "__main__":
    main()
