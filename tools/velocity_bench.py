"""Drive datum_ocean_displace with the velocity plane on, for a kernel trace of the velocity row and column passes beside the step's own
(DESIGN.md 5.16).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/velocity_bench.py --size 1024 --cascades 4

The trace's per-kernel statistics give each pass's mean duration per launch; the velocity pair against the step's row and column pass of
the same trace is the ratio DESIGN.md quotes.  Prints the byte budgets per point so that the ratio can be set against them."""

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
    ap.add_argument("--velocity", choices=("off", "on"), default="on")
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
        oc.set_velocity(args.velocity)
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
    print(f"velocity_bench N={N} C={C} velocity={args.velocity}: {t * 1e6:.1f} us per displace (wall), {launches} launches per pass of {group} cascades; "
          f"bytes per point: step 72, velocity pair 76 (4 + 8 + 24 written, 24 read + 16 written)")


if __name__ == "__main__":
    main()
