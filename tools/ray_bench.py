"""Drive the ray cast next to what a caller does without it for one kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o rays -- python tools/ray_bench.py
    python tools/ray_bench.py --split OUT/.../rays_kernel_trace.csv

On 1024^2 x 4 maps (wavescales 22, 64, 9.5, 140), 4 iterations, (S, R) = (32, 8), `--reps` casts per leg after a warm-up.  Two ray sets,
10^5 and 10^6 rays each:
  random   origins over 2 km x 2 km a few metres above or below the level, any direction from vertical to 2 degrees off horizontal
  fan      a camera's coherent fan: one origin 10 m above the water, a 1000-column grid of directions from 5 to 60 degrees below the horizon
and for each set and size, with 1 and with 4 cascades, in this order: the baseline, datum_ocean_cast_rays, the baseline again.  The baseline
is S + R + 2 launches of datum_ocean_sample_surface_blend on one point per ray (the rays' mid points: what a caller's host loop would
send; the kernel's time does not depend on which sample of the march they are) -- the launches alone, without the caller's host logic and
copies in between.  The spread between a baseline's two runs is what the cast is judged against.  Launch order is the order of the legs,
so --split cuts the trace's rows per leg."""

import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C, ITERATIONS, STEPS, REFINE = 1024, 4, 4, 32, 8
SCALES = [22.0, 64.0, 9.5, 140.0]
ONE, ALL = [0], [0, 1, 2, 3]
QUERY, RAYS = "ocean_surface_blend_kernel", "ocean_ray_kernel"
PER_CAST = STEPS + REFINE + 2

# (label, kernel name in the trace, cascade list, launches per repetition)
LEGS = [("queries x1", QUERY, ONE, PER_CAST), ("rays x1", RAYS, ONE, 1), ("queries x1 again", QUERY, ONE, PER_CAST),
        ("queries x4", QUERY, ALL, PER_CAST), ("rays x4", RAYS, ALL, 1), ("queries x4 again", QUERY, ALL, PER_CAST)]
SETS = [("random", 10 ** 5), ("random", 10 ** 6), ("fan", 10 ** 5), ("fan", 10 ** 6)]


def rays_of(which, n, rs):
    r = np.empty((n, 8), np.float32)
    if which == "random":
        el = np.radians(rs.uniform(2, 90, n)) * rs.choice([-1, 1], n)
        az = rs.uniform(0, 2 * np.pi, n)
        r[:, 0:2] = rs.uniform(-1000, 1000, (n, 2))
        r[:, 2] = 0.3 - np.sign(el) * rs.uniform(0.5, 4.0, n)                    # up-going rays start below, down-going above
        r[:, 4], r[:, 5], r[:, 6] = np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)
        r[:, 3] = 0.0
        r[:, 7] = rs.uniform(4.0, 8.0, n) / np.abs(np.sin(el))                  # far enough to reach the other side
    else:
        cols = 1000
        i, j = np.arange(n) % cols, np.arange(n) // cols
        az = np.radians(-30 + 60 * i / (cols - 1))
        el = -np.radians(5 + 55 * j / max(n // cols - 1, 1))
        r[:, 0:3] = (0.0, 0.0, 10.3)
        r[:, 4], r[:, 5], r[:, 6] = np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)
        r[:, 3] = 0.0
        r[:, 7] = 14.0 / np.abs(np.sin(el))
    return r


def run(args):
    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)
    with capi.Ocean(N, C) as oc:
        for c in range(C):
            oc.set_cascade(c, SCALES[c], 1.0)
            oc.upload_state(c, (rs.standard_normal((N, N, 2)) * (4e-3 / N)).astype(np.float32))
        oc.update(np.float32(1 / 60))
        oc.displace()
        s = capi.OceanSet()
        s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, 0.8, 0.5, 1.1
        s.swelldirection[:] = (0.780869, 0.624695)
        s.plane[:] = (0.0, 0.0, 1.0, -0.3)
        for which, n in SETS:
            rays = rays_of(which, n, rs)
            mid = 0.5 * (rays[:, 3] + rays[:, 7])
            dr = torch.from_numpy(rays).cuda()
            pts = torch.from_numpy(np.ascontiguousarray(rays[:, 0:2] + mid[:, None] * rays[:, 4:6])).cuda()
            recs = torch.empty(n * 12, dtype=torch.float32, device="cuda")
            out = torch.empty(n * 8, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            oc.sync()
            for label, kernel, cascades, per in LEGS:
                for _ in range((args.reps + 1) * per):
                    if kernel == QUERY:
                        oc.sample_surface_blend(cascades, s, pts.data_ptr(), n, out.data_ptr(), ITERATIONS)
                    else:
                        oc.cast_rays(cascades, s, dr.data_ptr(), n, recs.data_ptr(), ITERATIONS, STEPS, REFINE)
                oc.sync()
                print(f"ray_bench {which} {n} rays {label}: {(args.reps + 1) * per} launches")
            status = recs.cpu().numpy().reshape(n, 12)[:, 3]
            assert np.isfinite(status).all()
            print(f"ray_bench {which} {n} rays: miss {np.mean(status == 0):.3f}, enter {np.mean(status == 1):.3f}, leave {np.mean(status == 2):.3f}")


def split(args):
    """per-leg time of ONE cast (the baseline: the sum of its S + R + 2 launches) from the kernel_trace.csv of one run, the warm-up
    repetition of each leg dropped"""
    rows = []
    with open(args.split) as f:
        for r in csv.DictReader(f):
            for key in (QUERY, RAYS):
                if key in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), key, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
                    break
    rows = [(key, d) for _, key, d in sorted(rows)]          # launch order, whatever order the trace lists its rows in
    want = sum((args.reps + 1) * per for _, _, _, per in LEGS) * len(SETS)
    assert len(rows) == want, (len(rows), want)
    k = 0
    for which, n in SETS:
        print(f"{which}, {n} rays:")
        for label, kernel, _, per in LEGS:
            count = (args.reps + 1) * per
            chunk = rows[k:k + count]
            k += count
            assert all(name == kernel for name, _ in chunk), (label, kernel)
            d = np.array([t for _, t in chunk[per:]], np.float64).reshape(args.reps, per).sum(1) / 1e3
            print(f"{label:>20}: one cast = {per:2d} launch(es): mean {d.mean():10.2f} us, min {d.min():10.2f} us, max {d.max():10.2f} us over {len(d)} casts")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--split", help="kernel_trace.csv of a run: print the per-leg times instead of running")
    args = ap.parse_args()
    if args.split:
        split(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
