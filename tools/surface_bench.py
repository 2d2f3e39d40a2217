"""Drive datum_ocean_sample_surface for a kernel trace of ocean_surface_kernel (surface queries).

    rocprofv3 --kernel-trace --stats -d OUT -o surface -- python tools/surface_bench.py --size 1024
    rocprofv3 --kernel-trace --stats -d OUT -o surface -- python tools/surface_bench.py --size 4096

Per map size: 10^3, 10^5 and 10^6 random points over 2 km x 2 km (the base point of each lands anywhere in the repeated map), iterations
0 / 4 / 16, `--reps` launches each after a warm-up launch.  Launch order is the order of the legs, so the trace's kernel list can be
split per leg (the kernel is the same for every leg: the per-leg mean comes from the trace's rows, tools/surface_bench.py --split reads
its kernel_trace.csv).  Prints the byte budget of one query: 16 B of layer 0 per corner and evaluation, then 8 B of layer 1 and 4 B of
foam per corner, 8 B in, 32 B out."""

import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (10 ** 3, 10 ** 5, 10 ** 6)
ITERATIONS = (0, 4, 16)


def budget(iterations, foam):
    """(bytes through the caches, bytes to and from HBM) of one query"""
    cached = 4 * 16 * (iterations + 1) + 4 * 8 + (4 * 4 if foam else 0)
    return cached, 8 + 32


def legs():
    return [(m, it) for m in COUNTS for it in ITERATIONS]


def run(args):
    import torch

    from datum_amd import capi

    N = args.size
    rs = np.random.RandomState(1)
    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, 64.0, 1.35)
        h0 = (rs.standard_normal((N, N, 2)) * (4e-3 / N)).astype(np.float32)
        oc.upload_state(0, h0)
        oc.set_foam("jacobian")
        oc.update(np.float32(1 / 60))
        oc.displace()
        s = capi.OceanSet()
        s.swelllength, s.swellamplitude, s.swellsteepness = 40.0, 0.8, 0.4
        s.swelldirection[:] = (0.780869, 0.624695)
        s.scale = np.float32(1.0) / np.float32(64.0)
        s.plane[:] = (0.0, 0.0, 1.0, 0.0)
        pts = torch.from_numpy(rs.uniform(-1000, 1000, (max(COUNTS), 2)).astype(np.float32)).cuda()
        out = torch.empty(max(COUNTS) * 8, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        oc.sync()
        for m, it in legs():
            oc.sample_surface(0, s, pts.data_ptr(), m, out.data_ptr(), it)      # warm-up
            oc.sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                oc.sample_surface(0, s, pts.data_ptr(), m, out.data_ptr(), it)
            oc.sync()
            t = (time.perf_counter() - t0) / args.reps
            cached, hbm = budget(it, True)
            print(f"surface_bench N={N} points={m} iterations={it}: {t * 1e6:.1f} us per call (wall, enqueue-bound below ~1e5 points), "
                  f"budget {cached} B cached + {hbm} B HBM per query")


def split(args):
    """per-leg mean kernel time from a rocprofv3 kernel_trace.csv of one run (warm-up launch of each leg dropped)"""
    rows = []
    with open(args.split) as f:
        for r in csv.DictReader(f):
            if "ocean_surface_kernel" in r["Kernel_Name"]:
                rows.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    per = args.reps + 1
    assert len(rows) == per * len(legs()), (len(rows), per * len(legs()))
    for k, (m, it) in enumerate(legs()):
        d = np.array(rows[k * per + 1:(k + 1) * per], np.float64) / 1e3
        print(f"N={args.size} points={m:>8} iterations={it:>2}: mean {d.mean():8.2f} us, min {d.min():8.2f} us, max {d.max():8.2f} us over {len(d)} launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--split", help="kernel_trace.csv of a run: print the per-leg kernel means instead of running")
    args = ap.parse_args()
    if args.split:
        split(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
