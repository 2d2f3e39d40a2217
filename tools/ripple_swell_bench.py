"""Time ripple swell: the refresh of the forcing plane, and a sub-step with swell against its walled parent and its bed parent
(DESIGN.md 5.30).

    python tools/ripple_swell_bench.py [--reps 20] [--rounds 7] [--limit 180] [--out profiles/ripple_swell.txt]

Per R = 256 and R = 1024, in one process and on one handle with 1024 x 1024 maps x 4 cascades displaced twice from a random spectrum, over
a harbour of 64 walls (an 8 x 8 array of rotated boxes): datum_ocean_refresh_ripple_swell with all four cascades and 4 iterations; a call
of datum_ocean_step_ripples in the WAVE mode with the sponge on, 8 sub-steps per call, with walls alone (ocean_ripple_step_walls_kernel) and
then with the plane current (ocean_ripple_step_walls_swell_kernel); the same over a beach (ocean_ripple_bed_step_kernel against
ocean_ripple_bed_swell_step_kernel).  Every leg runs in a process of its own under a time limit of its own (`--limit` seconds); the first
leg that fails or runs out of time ends the run.  A round enqueues `reps` repetitions behind a sync and waits for them: wall-clock per
repetition, launch overhead included and overlapped.  One warm-up round, then `rounds` rounds; the median and the rounds' range.  The
lines are printed and written to `--out`."""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUBSTEPS, CELL, N, CASCADES, WALLS = 8, 1.0, 1024, 4, 64

from tools.ripple_bed_bench import beach  # noqa: E402


def harbour(capi, R):
    """64 boxes, each R / 25 by R / 100 cells, turned by 0.3 rad more than the last, on an 8 x 8 array over the window round the origin"""
    w = np.zeros(WALLS, capi.RIPPLE_WALL)
    for k in range(WALLS):
        i, j = k % 8, k // 8
        w[k]["center"] = ((i + 0.5) * R / 8 - R / 2) * CELL, ((j + 0.5) * R / 8 - R / 2) * CELL
        w[k]["axis"] = np.cos(0.3 * k), np.sin(0.3 * k)
        w[k]["half"] = R * CELL / 25, R * CELL / 100
        w[k]["kind"] = capi.RIPPLE_WALL_BOX
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
    return [float(np.median(t)), float(min(t)), float(max(t))]


def leg(R, reps, rounds):
    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)
    dt = float(np.float32(1 / 60))
    out = {"R": R}
    with capi.Ocean(N, CASCADES) as oc:
        for c in range(CASCADES):
            oc.set_cascade(c, 22.0 * 2.0 ** c, 1.0)
            oc.upload_state(c, (1e-4 * rs.standard_normal((N, N, 2))).astype(np.float32))
        for _ in range(2):
            oc.update(dt)
            oc.displace()
        s = capi.OceanSet()
        s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, 0.8, 0.5, 1.1
        s.swelldirection[:] = (0.780869, 0.624695)
        s.scale = np.float32(1.0 / 22.0)
        s.plane[:] = (0.0, 0.0, 1.0, -0.3)
        cascades = list(range(CASCADES))
        oc.set_ripple_dispersion(capi.RIPPLE_WAVE)
        oc.set_ripples(R, CELL)
        imp = np.zeros((4096, 4), np.float32)
        imp[:, :2], imp[:, 2] = rs.uniform(-R / 2, R / 2, (4096, 2)), rs.standard_normal(4096)
        di = torch.from_numpy(imp).cuda()
        oc.deposit_ripples(di.data_ptr(), len(imp))
        oc.set_ripple_walls(harbour(capi, R))
        out["wall_cells"] = int(oc.read_ripple_walls().sum())
        step = lambda k: oc.step_ripples(dt, SUBSTEPS)
        out["walls"] = timed(oc, step, reps, rounds)
        oc.set_ripple_swell(True)
        out["refresh"] = timed(oc, lambda k: oc.refresh_ripple_swell(cascades, s, 4), reps, rounds)
        out["boundary"] = int(np.count_nonzero(oc.read_ripple_swell()))
        assert oc.ripple_swell_device()[2]
        out["walls_swell"] = timed(oc, step, reps, rounds)
        oc.set_ripple_swell(False)
        bed, depths = beach(capi, R)
        oc.set_ripple_bed(bed, depths)
        out["bed"] = timed(oc, step, reps, rounds)
        oc.set_ripple_swell(True)
        out["bed_refresh"] = timed(oc, lambda k: oc.refresh_ripple_swell(cascades, s, 4), reps, rounds)
        out["bed_boundary"] = int(np.count_nonzero(oc.read_ripple_swell()))
        out["bed_swell"] = timed(oc, step, reps, rounds)
        out["finite"] = bool(np.isfinite(oc.read_ripples()).all())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=float, default=180.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ripple_swell.txt"))
    ap.add_argument("--leg", metavar="R", help="run one leg in this process and print its result as JSON")
    args = ap.parse_args()

    if args.leg:
        print(json.dumps(leg(int(args.leg), args.reps, args.rounds)))
        return 0

    lines = [f"ripple_swell_bench: {N} x {N} maps x {CASCADES}, a harbour of {WALLS} walls, {SUBSTEPS} sub-steps per step call, median [min - max] of {args.rounds} rounds of {args.reps}"]
    status = 0
    fmt = lambda v: f"{v[0]:8.1f} us [{v[1]:.1f} - {v[2]:.1f}]"
    for R in (256, 1024):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--rounds", str(args.rounds), "--leg", str(R)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"ripple_swell_bench R={R}: no result within {args.limit:.0f} s; stopping")
            status = 1
            break
        if done.returncode != 0:
            lines.append(f"ripple_swell_bench R={R}: exit status {done.returncode}; stopping\n{done.stderr[-2000:]}")
            status = 1
            break
        r = json.loads(done.stdout.strip().splitlines()[-1])
        lines.append(f"ripple_swell_bench R={R} refresh, 4 cascades, 4 iterations: walls {fmt(r['refresh'])} per call ({r['wall_cells']} wall cells, {r['boundary']} cells with a source); "
                     f"over the beach {fmt(r['bed_refresh'])} ({r['bed_boundary']} cells with a source)")
        lines.append(f"ripple_swell_bench R={R} step, walls: parent {fmt(r['walls'])}, swell {fmt(r['walls_swell'])} per call, swell / parent = {r['walls_swell'][0] / r['walls'][0]:.2f}")
        lines.append(f"ripple_swell_bench R={R} step, bed: parent {fmt(r['bed'])}, swell {fmt(r['bed_swell'])} per call, swell / parent = {r['bed_swell'][0] / r['bed'][0]:.2f}; finite {r['finite']}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
