#!/usr/bin/env python3
"""Three-receiver back-projection and the multi-baseline ATI resolver (sarx.tdbp_multi).

Three receive channels of the bistatic echo model (run_bistatic_physics_gpu, one call per receiver offset) are synthesised on the
device on the orbit arc of sar_batch_sim.py:262-268 (along track = x) with a short waveform (2 us, 50 MHz at 60 MHz sampling, PRF
5 kHz): six stationary scatterers and one mover with 16 m/s of ground-range speed, placed so that its radial speed brings its image
to the middle of the chip.  The receivers ride at (-d, +d, -d + 10 d), d = V / PRF: a short baseline of one pulse interval
(unambiguous to +-38.8 m/s) and a long one of five (+-7.8 m/s).  All three are back-projected onto ONE ground chip in one enqueue;
the short pair goes through sarx.gmti_detect, and every report is resolved on the device.  Prints, for the strongest report, the
speed the long baseline gives alone (wrapped: near -3.5 m/s, the wrong sign), the short baseline's, and the resolved one (near
12 m/s) against the geometry's.  With --relocate the resolved speed puts the report back on the ground (sarx.ground_relocate, DESIGN.md
4.21): the chip shows the mover near (0, 0) m, it is at (49.5 * speed, 0) m.

    python3 examples/sar_tdbp_multi_gpu.py [--pulses 320] [--speed 16] [--nx 90] [--ny 70] [--scene-size 360] [--relocate]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nis-sar-amtigmti-video_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pulses", type=int, default=320)
    ap.add_argument("--speed", type=float, default=16.0, help="ground-range speed of the mover, m/s")
    ap.add_argument("--nx", type=int, default=90)
    ap.add_argument("--ny", type=int, default=70)
    ap.add_argument("--scene-size", type=float, default=360.0)
    ap.add_argument("--relocate", action="store_true", help="also relocate the reports to their ground position by the resolved speed")
    a = ap.parse_args()
    import sarx
    kb = sarx.batch_constants()
    prf, fs, t_p, bw = 5000.0, 60e6, 2e-6, 50e6
    n_p = a.pulses
    t_vec = (np.arange(n_p) - n_p / 2) / prf
    pos, vel = sarx.orbit_arc(t_vec, kb)
    speed = float(np.linalg.norm(vel[n_p // 2]))
    d = speed / prf
    offs = (-d, d, 9 * d)
    rng = np.random.default_rng(11)
    still = [{"position": [float(rng.uniform(-120, 120)), float(rng.uniform(-120, 120)), 0.0], "rcs": float(rng.uniform(1.0, 50.0))}
             for _ in range(6)]
    v_m = np.array([0.0, a.speed, 0.0])
    p_m = np.array([49.5 * a.speed, 0.0, 0.0])                        # v_los R0 / V_ground of along-track shift, the other way
    los = (p_m - pos[n_p // 2]) / np.linalg.norm(p_m - pos[n_p // 2])
    v_true = float(np.dot(v_m, los))
    raws = []
    for off in offs:
        raw, t_start = sarx.run_bistatic_physics_gpu(still, t_vec, pos, vel, off, [0.0, 0.0, 0.0], FS=fs, BW=bw, T_p=t_p, R0=kb["R0"],
                                                     C=kb["C"], FC=kb["FC"], device=True)
        sarx.run_bistatic_physics_gpu([{"position": p_m.tolist(), "rcs": 50.0}], t_vec, pos, vel, off, v_m, FS=fs, BW=bw, T_p=t_p,
                                      R0=kb["R0"], C=kb["C"], FC=kb["FC"], device=True, add_to=raw)
        raws.append(raw)
    n_s = raws[0].shape[1]
    # run_bistatic_physics_gpu spaces its fast-time grid by window / (N - 1): the plan's sample rate follows it
    consts = dict(kb, FS=fs * (n_s - 1) / n_s, T_P=t_p, K_RATE=bw / t_p)
    res = sarx.tdbp_multi(raws, pos, vel, offs, t_start, n_s, t_vec, a.scene_size, a.nx, a.ny, consts=consts, device_output=True)
    lam = res.wavelength
    print(f"route {res.route}; lags {', '.join(f'{x * 1e6:.1f} us' for x in res.lags_s)}; unambiguous spans "
          f"{', '.join(f'+-{x:.2f} m/s' for x in res.v_ambiguity)}")
    short = res.pair(1)
    xs, ys = np.linspace(-a.scene_size / 2, a.scene_size / 2, a.nx), np.linspace(-a.scene_size / 2, a.scene_size / 2, a.ny)
    rep = sarx.gmti_detect(short.img1, short.img2, xs, ys, wavelength_m=lam, platform_speed_mps=speed, lag_s=short.lag_s, pfa=1e-3)
    if not len(rep):
        print("no report")
    else:
        rec = res.resolve(rep, v_max=30.0)
        r = int(np.argmax(rep.detections["power"]))
        det, best = rep.detections[r], rec[r]
        wrapped = -lam * best["phase"][1] / (4 * np.pi * res.lags_s[1])
        print(f"{len(rep)} reports; the strongest at ({xs[det['j']]:.1f}, {ys[det['i']]:.1f}) m")
        print(f"long baseline alone  : phase {best['phase'][1]:+.4f} rad -> v_los {wrapped:+.3f} m/s (wrapped)")
        print(f"short baseline alone : phase {best['phase'][0]:+.4f} rad -> v_los {best['v_coarse']:+.3f} m/s")
        print(f"resolved             : k = {best['k']}, v_los {best['v_los']:+.3f} m/s; cost {best['cost']:.2e}, the next wrap count's "
              f"{best['cost_next']:.3f}")
        print(f"geometry             : v_los {v_true:+.3f} m/s")
        if a.relocate:
            # the short pair's mean phase centre at the reference time; an output grid wide enough for the along-track displacement
            p_ref, v_ref = sarx.reference_geometry(pos, vel, t_vec, offs[:2])
            span = 2.0 * (abs(p_m[0]) + a.scene_size)
            out = sarx.ground_relocate(rep, rec["v_los"], valid=rec["status"], pos_ref=p_ref, vel_ref=v_ref, grid=(a.scene_size, a.nx, a.ny),
                                       out_grid=(-span / 2, -span / 2, 4.0, 4.0, int(span / 4) + 1, int(span / 4) + 1))
            g = out.records[r]
            print(f"relocated            : ({g['x']:.1f}, {g['y']:.1f}) m, moved by ({g['shift_x']:+.1f}, {g['shift_y']:+.1f}) m; status {g['status']}, "
                  f"{len(out.reports)} of {len(out)} reports on the ground grid")
            print(f"the mover is at      : ({p_m[0]:.1f}, {p_m[1]:.1f}) m")
    res.release()
    for r in raws:
        r.release()


if __name__ == "__main__":
    main()
