"""Time the ripple layer's kernels.

    python tools/ripple_bench.py [--reps 20] [--rounds 7]

Two legs of datum_ocean_step_ripples, R = 256 and R = 1024 with the sponge on, 8 sub-steps per call (eight launches and one memset), and
one of datum_ocean_deposit_body_ripples, 4096 bodies x 64 probes on 1024^2 maps, a list of 1 cascade, 4 iterations, into the 1024-cell
layer of 1 m cells that holds them all.  A round enqueues `reps` repetitions of a leg behind a sync and waits for them: wall-clock per
repetition, launch overhead included and overlapped.  One warm-up round, then `rounds` rounds per leg; median and min .. max are printed.
Under a kernel trace the same run gives the time per launch of ocean_ripple_step_kernel and ocean_ripple_wake_kernel."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, NB, PER, ITERATIONS, SUBSTEPS = 1024, 4096, 64, 4, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)
    bodies = np.zeros(NB, capi.BODY_DTYPE)
    bodies["rotation"] = np.eye(3, dtype=np.float32).ravel()
    bodies["position"] = np.stack([rs.uniform(-480, 480, NB), rs.uniform(-480, 480, NB), rs.uniform(-0.5, 0.2, NB)], 1)
    bodies["first"], bodies["count"], bodies["cap"] = np.arange(NB) * PER, PER, 1.0
    motions = np.zeros(NB, capi.BODY_MOTION_DTYPE)
    motions["linear"], motions["angular"] = rs.uniform(-3, 3, (NB, 3)), rs.uniform(-0.2, 0.2, (NB, 3))
    probes = np.zeros((NB * PER, 4), np.float32)
    g = np.linspace(-1.5, 1.5, 8)
    xx, yy = np.meshgrid(g, g)
    probes[:, 0], probes[:, 1], probes[:, 3] = np.tile(xx.ravel(), NB), np.tile(yy.ravel(), NB), 9.0 / PER

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
        oc.upload_state(0, (rs.standard_normal((N, N, 2)) * (4e-3 / N)).astype(np.float32))
        oc.set_velocity("on")
        for _ in range(2):
            oc.update(np.float32(1 / 60))
            oc.displace()
        oc.sync()
        s = capi.OceanSet()
        s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, 0.8, 0.5, 1.1
        s.swelldirection[:] = (0.780869, 0.624695)
        s.plane[:] = (0.0, 0.0, 1.0, -0.3)

        db = torch.from_numpy(bodies.view(np.uint8).reshape(NB, 64).copy()).cuda()
        dm = torch.from_numpy(motions.view(np.uint8).reshape(NB, 32).copy()).cuda()
        dp = torch.from_numpy(probes).cuda()
        rec = torch.empty(NB * 8, dtype=torch.float32, device="cuda")
        dt = float(np.float32(1 / 60))

        for R in (256, 1024):
            oc.set_ripples(R, 1.0)
            imp = np.zeros((4096, 4), np.float32)
            imp[:, :2], imp[:, 2] = rs.uniform(-R / 2, R / 2, (4096, 2)), rs.standard_normal(4096)
            di = torch.from_numpy(imp).cuda()
            oc.deposit_ripples(di.data_ptr(), len(imp))
            t = timed(oc, lambda: oc.step_ripples(dt, SUBSTEPS))
            state = oc.read_ripples()
            print(f"ripple_bench step R={R}, {SUBSTEPS} sub-steps per call: median {np.median(t):8.1f} us, min {t.min():8.1f} us, max {t.max():8.1f} us per call; "
                  f"{np.median(t) / SUBSTEPS:6.2f} us per sub-step; finite {bool(np.isfinite(state).all())}, max|eta| {float(np.abs(state[..., 0]).max()):.3g}")

        t = timed(oc, lambda: oc.deposit_body_ripples([0], s, db.data_ptr(), dm.data_ptr(), NB, dp.data_ptr(), NB * PER, dt, rec.data_ptr(), ITERATIONS))
        r = rec.cpu().numpy().reshape(NB, 8)
        print(f"ripple_bench wake {NB} bodies x {PER} probes, {N}^2 maps, list of 1, {ITERATIONS} iterations, R=1024: median {np.median(t):8.1f} us, min {t.min():8.1f} us, "
              f"max {t.max():8.1f} us per call; {float((r[:, 6] > 0).mean()):.2f} of the bodies wet, dropped quanta {int(r[:, 3].sum())}, finite {bool(np.isfinite(r).all())}")


if __name__ == "__main__":
    main()
