"""Time the ripple layer's step over a bed against its plain WAVE step, set_ripple_bed, and center_ripples with a bed on.

    python tools/ripple_bed_bench.py [--reps 20] [--rounds 7] [--limit 120]

Per R = 256 and R = 1024, in one process and on one handle: a call of datum_ocean_step_ripples in the WAVE mode with the sponge on,
8 sub-steps per call, first without a bed (the parent's kernel) and then over a 1024 x 1024 map of a beach with a surf zone
(ocean_ripple_bed_step_kernel); then datum_ocean_set_ripple_bed with that map (the host's scan of the map for values that are not finite,
three allocations, a blocking upload of 4 MiB and the raster launch), and datum_ocean_center_ripples alternating between two centres with
the bed set (the scroll and the raster).  Every leg runs in a process of its own under a time limit of its own (`--limit` seconds); the
first leg that fails or runs out of time ends the run.  A round enqueues `reps` repetitions behind a sync and waits for them: wall-clock
per repetition, launch overhead included and overlapped.  One warm-up round, then `rounds` rounds; medians."""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUBSTEPS, CELL, MAP = 8, 1.0, 1024


def beach(capi, R):
    """a MAP x MAP map over the window round the origin: 1.5 m of water that shoals to land towards +x, relief, a surf zone"""
    rs = np.random.RandomState(2)
    texel = R * CELL / (MAP - 1)
    x = -R * CELL / 2 + texel * np.arange(MAP)
    depths = (1.5 - 2.0 * np.clip((x[None, :] - 0.1 * R * CELL) / (0.35 * R * CELL), 0, 1) + 0.05 * rs.standard_normal((MAP, MAP))).astype(np.float32)
    bed = np.zeros(1, capi.RIPPLE_BED)[0]
    bed["width"], bed["height"], bed["origin"], bed["texel"] = MAP, MAP, (-R * CELL / 2, -R * CELL / 2), texel
    bed["outside"], bed["max_depth"], bed["dry_depth"], bed["surf_depth"], bed["surf_gamma"] = 1.5, 1.5, 0.05, 0.6, 2.0
    return bed, depths


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


def leg(R, reps, rounds):
    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)
    dt = float(np.float32(1 / 60))
    out = {"R": R}
    with capi.Ocean(64, 1) as oc:
        oc.set_cascade(0, 22.0, 1.0)
        oc.upload_state(0, np.zeros((64, 64, 2), np.float32))
        oc.set_ripple_dispersion(capi.RIPPLE_WAVE)
        oc.set_ripples(R, CELL)
        imp = np.zeros((4096, 4), np.float32)
        imp[:, :2], imp[:, 2] = rs.uniform(-R / 2, R / 2, (4096, 2)), rs.standard_normal(4096)
        di = torch.from_numpy(imp).cuda()
        oc.deposit_ripples(di.data_ptr(), len(imp))
        out["plain"] = timed(oc, lambda k: oc.step_ripples(dt, SUBSTEPS), reps, rounds)
        bed, depths = beach(capi, R)
        oc.set_ripple_bed(bed, depths)
        d, q = oc.read_ripple_bed()
        out["solid"], out["surf"] = int((d == 0).sum()), int((q > 0).sum())
        out["bed"] = timed(oc, lambda k: oc.step_ripples(dt, SUBSTEPS), reps, rounds)
        out["set"] = timed(oc, lambda k: oc.set_ripple_bed(bed, depths), reps, rounds)
        out["center"] = timed(oc, lambda k: oc.center_ripples(3.5 * CELL * (k & 1), -2.5 * CELL * (k & 1)), reps, rounds)
        out["finite"] = bool(np.isfinite(oc.read_ripples()).all())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--leg", metavar="R", help="run one leg in this process and print its result as JSON")
    args = ap.parse_args()

    if args.leg:
        print(json.dumps(leg(int(args.leg), args.reps, args.rounds)))
        return 0

    for R in (256, 1024):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--rounds", str(args.rounds), "--leg", str(R)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"ripple_bed_bench R={R}: no result within {args.limit:.0f} s; stopping")
            return 1
        if done.returncode != 0:
            print(f"ripple_bed_bench R={R}: exit status {done.returncode}; stopping\n{done.stderr[-2000:]}")
            return 1
        r = json.loads(done.stdout.strip().splitlines()[-1])
        print(f"ripple_bed_bench step R={R} WAVE, {SUBSTEPS} sub-steps per call: plain {r['plain']:8.1f} us, over a bed {r['bed']:8.1f} us per call "
              f"({r['solid']} solid cells, {r['surf']} in the surf zone), bed / plain = {r['bed'] / r['plain']:.2f}; finite {r['finite']}")
        print(f"ripple_bed_bench R={R}: set_ripple_bed with a {MAP} x {MAP} map {r['set']:.1f} us; center_ripples with the bed set {r['center']:.1f} us")
    return 0


if __name__ == "__main__":
    sys.exit(main())
