"""Drive body buoyancy next to the several-cascade query on the same world points for one kernel trace.

    rocprofv3 --kernel-trace --stats -d OUT -o body -- python tools/body_bench.py
    python tools/body_bench.py --split OUT/.../body_kernel_trace.csv

On 1024^2 x 4 maps (wavescales 22, 64, 9.5, 140), 4 iterations, `--reps` launches per leg after a warm-up launch.  Two fleets:
  10^4 bodies x 64 probes
  10^2 hulls x 6400 probes, each hull split into 64 bodies of 100 probes with the hull's pose
and for each fleet, in this order: datum_ocean_sample_surface_blend on the fleet's world points (tests/body64.py: world32) with 1 and with 4
cascades, datum_ocean_reduce_bodies with 1 and with 4, then the two query legs again: the spread between a query leg's two runs is what
the body legs are judged against.  Launch order is the order of the legs, so --split cuts the trace's rows per leg."""

import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, C, ITERATIONS = 1024, 4, 4
SCALES = [22.0, 64.0, 9.5, 140.0]
ONE, ALL = [0], [0, 1, 2, 3]
QUERY, BODY = "ocean_surface_blend_kernel", "ocean_body_kernel"

# (label, kernel name in the trace, cascade list)
LEGS = [("surface_blend x1", QUERY, ONE), ("surface_blend x4", QUERY, ALL), ("bodies x1", BODY, ONE), ("bodies x4", BODY, ALL),
        ("surface_blend x1 again", QUERY, ONE), ("surface_blend x4 again", QUERY, ALL)]
FLEETS = ["10^4 x 64", "10^2 x 6400 as 100s"]


def _rotations(rs, n):
    q = rs.standard_normal((n, 4))
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)


def fleet(which, rs):
    import body64

    if which == 0:
        poses, per, parts = 10 ** 4, 64, 1
    else:
        poses, per, parts = 10 ** 2, 100, 64
    rot = np.repeat(_rotations(rs, poses), parts, 0)
    pos = rs.uniform(-1000, 1000, (poses, 3))
    pos[:, 2] = rs.uniform(-1.5, 1.0, poses)
    pos = np.repeat(pos, parts, 0)
    nb = poses * parts
    bodies = body64.make_bodies(rot, pos, np.arange(nb) * per, [per] * nb, [2.0] * nb)
    probes = rs.uniform(-4, 4, (nb * per, 4)).astype(np.float32)
    probes[:, 3] = 0.25
    return bodies, probes


def run(args):
    import torch

    import body64
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
        for which, name in enumerate(FLEETS):
            bodies, probes = fleet(which, rs)
            w, _, bad = body64.world32(bodies, probes)
            assert not bad.any()
            nb, npr = len(bodies), len(probes)
            db = torch.from_numpy(bodies.view(np.uint8).reshape(nb, 64).copy()).cuda()
            dp = torch.from_numpy(probes).cuda()
            pts = torch.from_numpy(np.ascontiguousarray(w[:, :2])).cuda()
            recs = torch.empty(nb * 8, dtype=torch.float32, device="cuda")
            out = torch.empty(len(w) * 8, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            oc.sync()
            for label, kernel, cascades in LEGS:
                for _ in range(args.reps + 1):
                    if kernel == QUERY:
                        oc.sample_surface_blend(cascades, s, pts.data_ptr(), len(w), out.data_ptr(), ITERATIONS)
                    else:
                        oc.reduce_bodies(cascades, s, db.data_ptr(), nb, dp.data_ptr(), npr, recs.data_ptr(), ITERATIONS)
                oc.sync()
                print(f"body_bench {name} ({nb} bodies, {npr} probes) {label}: {args.reps + 1} launches")
            assert np.isfinite(recs.cpu().numpy()).all()


def split(args):
    """per-leg mean kernel time from the kernel_trace.csv of one run (the warm-up launch of each leg dropped)"""
    rows = []
    with open(args.split) as f:
        for r in csv.DictReader(f):
            for key in (QUERY, BODY):
                if key in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), key, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
                    break
    rows = [(key, d) for _, key, d in sorted(rows)]          # launch order, whatever order the trace lists its rows in
    per = args.reps + 1
    assert len(rows) == per * len(LEGS) * len(FLEETS), (len(rows), per * len(LEGS) * len(FLEETS))
    k = 0
    for name in FLEETS:
        print(f"{name}:")
        for label, kernel, _ in LEGS:
            chunk = rows[k * per:(k + 1) * per]
            k += 1
            assert all(n == kernel for n, _ in chunk), (label, kernel)
            d = np.array([t for _, t in chunk[1:]], np.float64) / 1e3
            print(f"{label:>24}: mean {d.mean():8.2f} us, min {d.min():8.2f} us, max {d.max():8.2f} us over {len(d)} launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--split", help="kernel_trace.csv of a run: print the per-leg kernel means instead of running")
    args = ap.parse_args()
    if args.split:
        split(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
