#!/usr/bin/env python3
"""The focus-velocity search on the pair per GMTI report against what a user could do before it: one whole-grid
sarx_tdbp_pair_dev per hypothesis (include/sarx_tdbp_pair_search.h).

The script's own waveform (batch_constants(): 22004 samples, 12000-tap chirp), 2500 pulses, two channels resident on the device
(two spotlight echoes synthesised there: the time of a launch does not depend on what the samples hold), a 512 x 512 grid of 1 m
pixels, 16 reports spread over it in a device slot that holds exactly them, chips of 32 x 32 pixels, 33 hypotheses along track.
In one process, on one plan and lane, timed with the lane's events after a warm-up, medians of rounds:

    search           one sarx_tdbp_pair_search_dev: two compressions, 16 x 33 chips of both channels, records, best
    search chips     the same with the chips written
    search n_hyp 1   one hypothesis: the fixed cost, two compressions above all
    pair x n_hyp     n_hyp whole-grid sarx_tdbp_pair_dev calls (complex64 pair): the yardstick.  It compresses both channels n_hyp
                     times and images every pixel of the grid; the sharpness of each chip would still have to be taken on the host.

Prints one JSON line (and writes it to --out).

    python3 tools/bench_tdbp_pair_search.py [--pulses 2500] [--grid 512] [--reports 16] [--chip 32] [--hyps 33] [--rounds 5] [--out FILE.json]"""
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
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--reports", type=int, default=16)
    ap.add_argument("--chip", type=int, default=32)
    ap.add_argument("--hyps", type=int, default=33)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    from sarx import _ffi, slot, tdbp
    from sarx.tdbp_pair import pair_params
    from sarx.tdbp_pair_search import BEST_DTYPE, search_params
    from sarx.tdbp_search import RECORD_DTYPE
    ctx = sarx.default_context()
    k = sarx.batch_constants()
    n_p, nx, md, n_hyp = a.pulses, a.grid, a.reports, a.hyps
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
    hyps = np.ascontiguousarray(sarx.tdbp_velocity_line((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 16.0, n_hyp))
    rep = np.zeros(md, slot.REPORT_DTYPE)
    rep["i"], rep["j"] = rng.integers(0, nx, md), rng.integers(0, nx, md)
    d_slot = ctx.to_device(slot.encode(rep, md))
    swath = float(nx)
    plan = tdbp.cached_plan(ctx, k, n_p, n_s, nx, nx)
    n_chip = a.chip * a.chip
    d_rec, d_best = ctx.alloc(md * n_hyp * RECORD_DTYPE.itemsize), ctx.alloc(md * BEST_DTYPE.itemsize)
    d_chips, d64 = ctx.alloc(md * n_hyp * 2 * n_chip * 16), ctx.alloc(16 * nx * nx)

    def search(n, chips=False):
        sp = search_params((a.chip, a.chip), n, "dpca")
        _ffi.check(ctx.lib.sarx_tdbp_pair_search_dev(plan.h, raws[0].ptr, raws[1].ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t0),
                                                     swath, C.byref(prm), hyps.ctypes.data, d_slot.ptr + slot.HEADER_BYTES, d_slot.ptr, md,
                                                     C.byref(sp), d_rec.ptr, d_best.ptr, d_chips.ptr if chips else None), ctx.h)

    def pairs():
        for h in range(n_hyp):
            _ffi.check(ctx.lib.sarx_tdbp_pair_dev(plan.h, raws[0].ptr, raws[1].ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t0),
                                                  hyps[h].ctypes.data, swath, C.byref(prm), None, d64.ptr), ctx.h)

    out = {"device": ctx.info()["name"], "pulses": n_p, "num_samples": int(n_s), "grid": [nx, nx], "reports": md, "chip": [a.chip, a.chip],
           "n_hyp": n_hyp}
    out["search_ms"], out["search_ms_rounds"] = _median_ms(ctx, lambda: search(n_hyp), a.rounds, a.reps)
    out["search_window"] = list(plan.last_window())
    tile = C.c_int()
    _ffi.check(ctx.lib.sarx_tdbp_pair_search_route(plan.h, C.byref(tile)), ctx.h)
    out["search_route"] = "tile" if tile.value else "exact"
    best = d_best.download(np.uint8, (md * BEST_DTYPE.itemsize,)).view(BEST_DTYPE)
    out["reports_inside"] = int(np.sum(best["k_best"] >= 0))
    out["search_chips_ms"], _ = _median_ms(ctx, lambda: search(n_hyp, True), a.rounds, a.reps)
    out["search_one_hyp_ms"], out["search_one_hyp_ms_rounds"] = _median_ms(ctx, lambda: search(1), a.rounds, a.reps)
    out["pairs_ms"], out["pairs_ms_rounds"] = _median_ms(ctx, pairs, a.rounds, 1)
    out["pairs_window"] = list(plan.last_window())
    _ffi.check(ctx.lib.sarx_tdbp_pair_route(plan.h, C.byref(tile)), ctx.h)
    out["pairs_route"] = "tile" if tile.value else "exact"
    out["pairs_over_search"] = round(out["pairs_ms"] / out["search_ms"], 2)
    out["search_ns_per_pixel_pulse_channel"] = round((out["search_ms"] - out["search_one_hyp_ms"]) * 1e6 / (2.0 * n_p * md * (n_hyp - 1) * n_chip), 6) \
        if n_hyp > 1 else None
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    for b in (*raws, d_slot, d_rec, d_best, d_chips, d64):
        b.release()


if __name__ == "__main__":
    main()
