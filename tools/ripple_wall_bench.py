"""Time the ripple layer's walled steps against its unwalled ones, the raster, and center_ripples with walls on.

    python tools/ripple_wall_bench.py [--reps 20] [--rounds 7] [--limit 120]

Per R = 256 and R = 1024 and per mode (DATUM_OCEAN_RIPPLE_WAVE, DATUM_OCEAN_RIPPLE_DEEP), in one process and on one handle: a call of
datum_ocean_step_ripples with the sponge on, 8 sub-steps per call, first without walls (the parent's kernels) and then with a harbour of
boxes set (ocean_ripple_step_walls_kernel / ocean_ripple_deep_step_walls_kernel); then datum_ocean_set_ripple_walls with 1, 64 and 256
records (the raster launch, a blocking upload of the list and two allocations), and datum_ocean_center_ripples alternating between two
centres with 64 records set (the scroll and the raster).  Every leg runs in a process of its own under a time limit of its own
(`--limit` seconds); the first leg that fails or runs out of time ends the run.  A round enqueues `reps` repetitions behind a sync and
waits for them: wall-clock per repetition, launch overhead included and overlapped.  One warm-up round, then `rounds` rounds; medians."""

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


def harbour(capi, R, count, rs):
    """`count` boxes inside the window round the origin: quays along the axes and piles, a tenth of a window long at the most"""
    w = np.zeros(count, capi.RIPPLE_WALL)
    ang = rs.uniform(0, 2 * np.pi, count)
    w["center"] = rs.uniform(-R / 2, R / 2, (count, 2)) * CELL
    w["axis"] = np.stack([np.cos(ang), np.sin(ang)], 1)
    w["half"] = np.stack([rs.uniform(1, R / 20, count), rs.uniform(0.6, 2, count)], 1) * CELL
    w["kind"] = capi.RIPPLE_WALL_BOX
    return w


def timed(oc, call, reps, rounds):
    t = []
    for rnd in range(rounds + 1):
        oc.sync()
        t0 = time.perf_counter()
        for k in range(reps):
            call(k)
        oc.sync()
        if rnd:
            t.append((time.perf_counter() - t0) / reps * 1e6)
    return float(np.median(t))


def leg(R, mode, reps, rounds):
    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)
    dt = float(np.float32(1 / 60))
    out = {"R": R, "mode": mode}
    with capi.Ocean(64, 1) as oc:
        oc.set_cascade(0, 22.0, 1.0)
        oc.upload_state(0, np.zeros((64, 64, 2), np.float32))
        oc.set_ripple_dispersion(capi.RIPPLE_DEEP if mode == "deep" else capi.RIPPLE_WAVE)
        oc.set_ripples(R, CELL)
        imp = np.zeros((4096, 4), np.float32)
        imp[:, :2], imp[:, 2] = rs.uniform(-R / 2, R / 2, (4096, 2)), rs.standard_normal(4096)
        di = torch.from_numpy(imp).cuda()
        oc.deposit_ripples(di.data_ptr(), len(imp))
        out["open"] = timed(oc, lambda k: oc.step_ripples(dt, SUBSTEPS), reps, rounds)
        lists = {n: harbour(capi, R, n, rs) for n in (1, 64, 256)}
        oc.set_ripple_walls(lists[64])
        out["cells"] = int(oc.read_ripple_walls().sum())
        out["walled"] = timed(oc, lambda k: oc.step_ripples(dt, SUBSTEPS), reps, rounds)
        for n, w in lists.items():
            out[f"raster{n}"] = timed(oc, lambda k: oc.set_ripple_walls(w), reps, rounds)
        oc.set_ripple_walls(lists[64])
        out["center"] = timed(oc, lambda k: oc.center_ripples(3.5 * CELL * (k & 1), -2.5 * CELL * (k & 1)), reps, rounds)
        out["finite"] = bool(np.isfinite(oc.read_ripples()).all())
    return out


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

    for R in (256, 1024):
        for mode in ("wave", "deep"):
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--rounds", str(args.rounds), "--leg", str(R), mode]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(f"ripple_wall_bench R={R} {mode}: no result within {args.limit:.0f} s; stopping")
                return 1
            if done.returncode != 0:
                print(f"ripple_wall_bench R={R} {mode}: exit status {done.returncode}; stopping\n{done.stderr[-2000:]}")
                return 1
            r = json.loads(done.stdout.strip().splitlines()[-1])
            print(f"ripple_wall_bench step R={R} {mode.upper()}, {SUBSTEPS} sub-steps per call: open {r['open']:8.1f} us, walled {r['walled']:8.1f} us per call "
                  f"({r['cells']} wall cells), walled / open = {r['walled'] / r['open']:.2f}; finite {r['finite']}")
            print(f"ripple_wall_bench R={R} {mode.upper()}: set_ripple_walls 1 / 64 / 256 records {r['raster1']:.1f} / {r['raster64']:.1f} / {r['raster256']:.1f} us; "
                  f"center_ripples with 64 records {r['center']:.1f} us")
    return 0


if __name__ == "__main__":
    sys.exit(main())
