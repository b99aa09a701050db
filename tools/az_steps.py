#!/usr/bin/env python3
"""Each of the four steps of the 16384^2 four-step azimuth transform alone (sarx_csa_pass ids 110-113: forward A with the
four-step twiddle, forward B with Phi_1, inverse A with the twiddle, inverse B with 1/n and the max slot armed), timed with a
host clock around `reps` launches that ends in a device synchronise.  Every configuration gets its own plan (SARX_AZ_IMPL and
SARX_AZ_WAVES are read at plan creation); the configurations are interleaved round by round so that drift hits them alike.

    python3 tools/az_steps.py [--n 16384] [--reps 40] [--rounds 3] [--configs old,wave1,wave4]

One JSON line: per configuration and step, the per-launch time of each round (ms) and their median."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))

CONFIGS = {"old": {"SARX_AZ_IMPL": "0"}, "wave1": {"SARX_AZ_IMPL": "1", "SARX_AZ_WAVES": "1"},
           "wave4": {"SARX_AZ_IMPL": "1", "SARX_AZ_WAVES": "4"}}
STEPS = {110: "fwd_A_twiddle", 111: "fwd_B_phi1", 112: "inv_A_twiddle", 113: "inv_B_scale"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="old,wave1,wave4")
    a = ap.parse_args()
    import sarx
    from sarx import _ffi, radar
    ctx = sarx.default_context()
    n = a.n
    px = n * n
    args = radar.focus_args(n)
    plans = {}
    for name in a.configs.split(","):
        saved = {k: os.environ.get(k) for k in CONFIGS[name]}
        os.environ.update(CONFIGS[name])
        plans[name] = sarx.CsaPlan(ctx, n, n, *args, flags=_ffi.FUSE_RANGE)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    x, y = ctx.alloc(px * 8), ctx.alloc(px * 8)
    d_max = ctx.alloc(_ffi.MAX_SLOT_BYTES)
    for p in plans.values():
        p.set_max_slot(d_max)
    ctx.fill_noise(x, px, 20261016)
    res = {name: {s: [] for s in STEPS.values()} for name in plans}
    for name, p in plans.items():          # warm-up: every kernel loaded once
        for pid in STEPS:
            p.run_pass(pid, x, y)
    ctx.sync()
    for _ in range(a.rounds):
        for name, p in plans.items():
            for pid, step in STEPS.items():
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    p.run_pass(pid, x, y)
                ctx.sync()
                res[name][step].append(round((time.perf_counter() - t0) * 1e3 / a.reps, 4))
    out = {"n": n, "reps": a.reps, "env": {k: v for k, v in os.environ.items() if k.startswith("SARX_")},
           "ms_per_launch": res,
           "median_ms": {name: {s: statistics.median(v) for s, v in r.items()} for name, r in res.items()},
           "sum_of_medians_ms": {name: round(sum(statistics.median(v) for v in r.values()), 4) for name, r in res.items()}}
    print(json.dumps(out))
    for b in (x, y, d_max):
        b.release()
    for p in plans.values():
        p.close()


if __name__ == "__main__":
    main()
