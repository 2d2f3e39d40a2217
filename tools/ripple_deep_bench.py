"""Time the ripple layer's DEEP step against its WAVE step.

    python tools/ripple_deep_bench.py [--reps 20] [--rounds 7] [--limit 120]

Four legs of datum_ocean_step_ripples with the sponge on, 8 sub-steps per call (eight launches and one memset): R = 256 and R = 1024, each in
DATUM_OCEAN_RIPPLE_WAVE (ocean_ripple_step_kernel, the parent's device code) and in DATUM_OCEAN_RIPPLE_DEEP (ocean_ripple_deep_step_kernel).
Every leg runs in a process of its own under a time limit of its own (`--limit` seconds); the first leg that fails or runs out of time
ends the run.  A round enqueues `reps` repetitions of the call behind a sync and waits for them: wall-clock per repetition, launch overhead
included and overlapped.  One warm-up round, then `rounds` rounds; median and min .. max are printed, then DEEP / WAVE per R."""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUBSTEPS, CELL = 8, 1.0


def leg(R, mode, reps, rounds):
    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)
    dt = float(np.float32(1 / 60))
    with capi.Ocean(64, 1) as oc:
        oc.set_cascade(0, 22.0, 1.0)
        oc.upload_state(0, np.zeros((64, 64, 2), np.float32))
        oc.set_ripple_dispersion(capi.RIPPLE_DEEP if mode == "deep" else capi.RIPPLE_WAVE)
        oc.set_ripples(R, CELL)
        imp = np.zeros((4096, 4), np.float32)
        imp[:, :2], imp[:, 2] = rs.uniform(-R / 2, R / 2, (4096, 2)), rs.standard_normal(4096)
        di = torch.from_numpy(imp).cuda()
        oc.deposit_ripples(di.data_ptr(), len(imp))
        t = []
        for rnd in range(rounds + 1):
            oc.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                oc.step_ripples(dt, SUBSTEPS)
            oc.sync()
            if rnd:
                t.append((time.perf_counter() - t0) / reps * 1e6)
        state = oc.read_ripples()
    t = np.array(t)
    return {"R": R, "mode": mode, "median": float(np.median(t)), "min": float(t.min()), "max": float(t.max()), "finite": bool(np.isfinite(state).all()),
            "eta": float(np.abs(state[..., 0]).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--leg", nargs=2, metavar=("R", "MODE"), help="run one leg in this process and print its result as JSON")
    args = ap.parse_args()

    if args.leg:
        print(json.dumps(leg(int(args.leg[0]), args.leg[1], args.reps, args.rounds)))
        return 0

    median = {}
    for R in (256, 1024):
        for mode in ("wave", "deep"):
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--rounds", str(args.rounds), "--leg", str(R), mode]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(f"ripple_deep_bench R={R} {mode}: no result within {args.limit:.0f} s; stopping")
                return 1
            if done.returncode != 0:
                print(f"ripple_deep_bench R={R} {mode}: exit status {done.returncode}; stopping\n{done.stderr[-2000:]}")
                return 1
            r = json.loads(done.stdout.strip().splitlines()[-1])
            median[R, mode] = r["median"]
            print(f"ripple_deep_bench step R={R} {mode.upper()}, {SUBSTEPS} sub-steps per call: median {r['median']:8.1f} us, min {r['min']:8.1f} us, max {r['max']:8.1f} us per call; "
                  f"{r['median'] / SUBSTEPS:7.2f} us per sub-step; finite {r['finite']}, max|eta| {r['eta']:.3g}")
        print(f"ripple_deep_bench R={R}: DEEP / WAVE = {median[R, 'deep'] / median[R, 'wave']:.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
