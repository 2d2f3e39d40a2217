"""Drive datum_ocean_displace with the foam plane on, for a kernel trace of ocean_foam_kernel (foam).

    rocprofv3 --kernel-trace --stats -d OUT -o foam -- python tools/foam_bench.py --size 1024 --cascades 4 --mode accumulate

Only the launches of the timed loop matter: the trace's per-kernel statistics give the foam kernel's mean duration per launch.
Prints the byte budget per launch (16 B read + 4 B written per point; ACCUMULATE reads 4 more) so that the fraction of 8 TB/s can be
formed from the trace."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--cascades", type=int, default=4)
    ap.add_argument("--mode", choices=("off", "jacobian", "accumulate"), default="jacobian")
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()

    from datum_amd import capi

    N, C = args.size, args.cascades
    rs = np.random.RandomState(1)
    with capi.Ocean(N, C) as oc:
        for c in range(C):
            oc.set_cascade(c, 22.0 * (c + 1), 1.35)
            h0 = (rs.standard_normal((N, N, 2)) * (1e-3 / N)).astype(np.float32)
            oc.upload_state(c, h0)
        oc.set_foam(args.mode)
        for _ in range(10):
            oc.update(np.float32(1 / 60))
            oc.displace()
        oc.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            oc.update(np.float32(1 / 60))
            oc.displace()
        oc.sync()
        t = (time.perf_counter() - t0) / args.steps
        group, launches = oc.cascade_group()
    per_point = 0 if args.mode == "off" else (24 if args.mode == "accumulate" else 20)
    print(f"foam_bench N={N} C={C} mode={args.mode}: {t * 1e6:.1f} us per displace (wall), {launches} foam launches of {group} cascades, "
          f"budget {per_point * N * N * group / 1e6:.1f} MB per launch")


if __name__ == "__main__":
    main()
