#!/usr/bin/env python3
"""Phase-gradient autofocus timings on the GPU (include/sarx_pga.h) at the VideoSAR loop's own shape: a stack of 46 frames of
512 x 512, four iterations, resident on the device, timed with lane events in rounds (medians of the rounds after a warm-up).

    python3 tools/bench_pga.py [--frames 46] [--size 512] [--iters 4] [--rounds 5] [--reps 3] [--out FILE.json]

Two ways over the same frames: one sarx_pga_dev on the stack, and one sarx_pga_dev per frame (46 calls into the same buffers).  The
apply launch alone is timed too.  Each figure comes with the bytes the algorithm has to move - (n_iter + 1) estimate reads of the
stack, n_iter apply reads and writes, and the tiles' partial rows written by every estimate launch and read by every integrate
launch - and the time those bytes take at COPY_TBPS (the best copy this part reaches, README).  The frames are seeded clutter with
point targets under a known phase error, so the run also says what was recovered.  Prints one JSON line (and writes it to --out)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nis-sar-amtigmti-video_amd"))

COPY_TBPS = 6.0


def frames_with_error(n_frames, n, seed=7):
    """(stack complex64 [n_frames x n x n], the injected phase [n]): unit clutter, 24 targets 30 dB above it per frame, the
    phase 6 x^2 (line removed) put on every frame's azimuth spectrum."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.0, 1.0, n)
    phi = 6.0 * x * x
    phi -= np.polyval(np.polyfit(x, phi, 1), x)
    w = np.exp(1j * np.fft.ifftshift(phi))[:, None]
    stack = np.empty((n_frames, n, n), np.complex64)
    for f in range(n_frames):
        img = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(2.0)
        cols = rng.choice(n, size=24, replace=False)
        img[rng.integers(0, n, size=24), cols] += 10.0 ** 1.5 * np.exp(2j * np.pi * rng.random(24))
        stack[f] = np.fft.ifft(np.fft.fft(img, axis=0) * w, axis=0)
    return stack, phi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=46)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sarx
    K = importlib.import_module("sarx.pga")
    ctx = sarx.default_context()
    nf, n, it = a.frames, a.size, a.iters
    stack, phi = frames_with_error(nf, n)
    prm = sarx.PgaParams(n_iter=it, power_floor=0.0)
    cp = prm.c_params(n)
    px = n * n
    d_in, d_out = ctx.to_device(stack), ctx.alloc(nf * px * 8)
    d_ph, d_rec = ctx.alloc(nf * n * 8), ctx.alloc(nf * (it + 1) * 32)
    d_ws = ctx.alloc(K.workspace_bytes(cp, n, n, n, nf, px))
    ws_frame = K.workspace_bytes(cp, n, n, n, 1, 0)

    def as_stack():
        K.enqueue(ctx, d_in.ptr, d_out.ptr, n, n, n, nf, px, cp, d_ph.ptr, d_rec.ptr, d_ws.ptr)

    def per_frame():
        for f in range(nf):
            K.enqueue(ctx, d_in.ptr + f * px * 8, d_out.ptr + f * px * 8, n, n, n, 1, 0, cp, d_ph.ptr + f * n * 8,
                      d_rec.ptr + f * (it + 1) * 32, d_ws.ptr + f * ws_frame)

    def apply_only():
        K.enqueue_apply(ctx, d_in.ptr, d_out.ptr, n, n, n, nf, px, d_ph.ptr, n, -1)

    frame_bytes = px * 8
    partial = ws_frame * 2                                  # written by the estimate launch, read by the integrate launch
    need = {"stack": nf * ((it + 1) * frame_bytes + it * 2 * frame_bytes + (it + 1) * partial),
            "per_frame": nf * ((it + 1) * frame_bytes + it * 2 * frame_bytes + (it + 1) * partial),
            "apply_only": nf * 2 * frame_bytes}
    steps = {"stack": as_stack, "per_frame": per_frame, "apply_only": apply_only}
    for fn in steps.values():                               # warm-up: code objects
        fn()
    ctx.sync()
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            ctx.record(0)
            for _ in range(a.reps):
                fn()
            ctx.record(1)
            ctx.sync()
            times[k].append(ctx.elapsed_ms(0, 1) / a.reps)
    as_stack()
    rec = np.array(d_rec.download(np.uint8, (nf * (it + 1) * 32,))).view(K.RECORD_DTYPE).reshape(nf, it + 1)
    ph = np.array(d_ph.download(np.float64, (nf, n)))
    x = np.arange(n) - n // 2
    resid = ph - phi[None, :]
    resid -= np.stack([np.polyval(np.polyfit(x, r, 1), x) for r in resid])
    sharp = rec["s4"] / rec["s2"] ** 2
    out = {"device": ctx.info()["name"], "frames": nf, "size": n, "n_iter": it, "copy_TBps": COPY_TBPS, "launches_per_call": 3 * it + 2,
           "recovered": {"residual_rms_rad_max": round(float(np.sqrt((resid ** 2).mean(axis=1)).max()), 4),
                         "final_rms_phase_max": float(rec[:, -1]["rms_phase"].max()),
                         "sharpness_before_median": float(np.median(sharp[:, 0])), "sharpness_after_median": float(np.median(sharp[:, -1]))}}
    for k in steps:
        med = float(np.median(times[k]))
        floor = need[k] / (COPY_TBPS * 1e12) * 1e3
        out[k] = {"ms_median": round(med, 4), "ms_rounds": [round(t, 4) for t in times[k]], "ms_per_frame": round(med / nf, 5),
                  "bytes_needed": int(need[k]), "GBps": round(need[k] / (med * 1e-3) / 1e9, 1), "floor_ms": round(floor, 4),
                  "fraction_of_floor": round(floor / med, 3)}
    for b in (d_in, d_out, d_ph, d_rec, d_ws):
        b.release()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
