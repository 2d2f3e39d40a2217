"""Time wake foam's update beside the ripple step it shares its form and bytes with.

    python tools/ripple_foam_bench.py [--reps 20] [--rounds 7]

Per R = 256 and R = 1024, two legs on one handle and one layer, 8 launches per call each: datum_ocean_step_ripples with 8 sub-steps (the
first takes the deposits in and is followed by a memset; the other seven are ocean_ripple_step_kernel<false>), and 8 calls of
datum_ocean_step_ripple_foam.  A round enqueues `reps` repetitions of a leg behind a sync and waits for them: wall-clock per repetition,
launch overhead included and overlapped.  One warm-up round, then `rounds` rounds per leg; median and min .. max are printed.  Under a
kernel trace the same run gives the time per launch of ocean_ripple_foam_kernel and of ocean_ripple_step_kernel<false>, whose ratio is
the figure DESIGN.md records."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, LAUNCHES = 64, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)

    def timed(oc, fn):
        t = []
        for rnd in range(args.rounds + 1):
            oc.sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            oc.sync()
            if rnd:
                t.append((time.perf_counter() - t0) / args.reps * 1e6)
        return np.array(t)

    with capi.Ocean(N, 1) as oc:
        oc.set_cascade(0, 22.0, 1.0)
        oc.upload_state(0, np.zeros((N, N, 2), np.float32))
        dt = float(np.float32(1 / 60))

        def foam():
            for _ in range(LAUNCHES):
                oc.step_ripple_foam(dt)

        for R in (256, 1024):
            oc.set_ripples(R, 1.0)
            oc.set_ripple_foam(True)
            imp = np.zeros((4096, 4), np.float32)
            imp[:, :2], imp[:, 2] = rs.uniform(-R / 2, R / 2, (4096, 2)), rs.standard_normal(4096)
            di = torch.from_numpy(imp).cuda()
            oc.deposit_ripples(di.data_ptr(), len(imp))
            ts = timed(oc, lambda: oc.step_ripples(dt, LAUNCHES))
            tf = timed(oc, foam)
            state, plane = oc.read_ripples(), oc.read_ripple_foam()
            for name, t in (("step", ts), ("foam", tf)):
                print(f"ripple_foam_bench {name} R={R}, {LAUNCHES} launches per call: median {np.median(t):8.1f} us, min {t.min():8.1f} us, max {t.max():8.1f} us per call; "
                      f"{np.median(t) / LAUNCHES:6.2f} us per launch")
            print(f"ripple_foam_bench R={R}: foam / step = {np.median(tf) / np.median(ts):.3f} (wall-clock medians); finite {bool(np.isfinite(state).all() and np.isfinite(plane).all())}, "
                  f"max|eta| {float(np.abs(state[..., 0]).max()):.3g}, covered cells {int(np.count_nonzero(plane))}, plane in [{float(plane.min()):.3g}, {float(plane.max()):.3g}]")


if __name__ == "__main__":
    main()
