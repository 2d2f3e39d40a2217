"""Time coupled stepping next to the three calls it replaces.

    python tools/couple_bench.py [--reps 20] [--rounds 7]

4096 bodies x 64 probes on 1024^2 maps, ripple layers of R = 256 and 1024 (cells of 4 m and 1 m: the fleet lies inside either window),
lists of 1 and of 4 cascades, 4 iterations, device arrays only.  Legs per layer and list, with h = dt / substeps:
  (a) datum_ocean_deposit_body_ripples(h) + datum_ocean_step_ripples(h, 1) + datum_ocean_step_bodies(h, 1)      one sub-step
  (b) datum_ocean_step_bodies_coupled, substeps = 1
  (a) x 4 and (c) datum_ocean_step_bodies_coupled, substeps = 4
(a) is not the same arithmetic -- its bodies do not feel the layer -- but it is what a caller ran before, with two solves per probe.
A round enqueues `reps` repetitions of a leg behind a sync and waits for them: wall-clock per repetition, launch overhead included and
overlapped.  One warm-up round, then `rounds` rounds per leg, the legs interleaved; median and min .. max over the rounds are printed.
Bodies and layer are reset before every round so that each leg sees the same state."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C, NB, PER, ITERATIONS = 1024, 4, 4096, 64, 4
SCALES = (22.0, 67.0, 211.0, 677.0)
LAYERS = ((256, 4.0), (1024, 1.0))


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
    motions["linear"], motions["angular"] = rs.uniform(-1, 1, (NB, 3)), rs.uniform(-0.2, 0.2, (NB, 3))
    motions["cl"], motions["cq"] = 5000.0, 200.0
    props = np.zeros(NB, capi.BODY_PROPS_DTYPE)
    props["invmass"], props["invinertia"], props["gravity"], props["buoyancy"] = 1 / 4000.0, 1 / 3000.0, 9.81, 9810.0
    probes = np.zeros((NB * PER, 4), np.float32)
    g = np.linspace(-1.5, 1.5, 8)
    xx, yy = np.meshgrid(g, g)
    probes[:, 0], probes[:, 1], probes[:, 3] = np.tile(xx.ravel(), NB), np.tile(yy.ravel(), NB), 9.0 / PER

    with capi.Ocean(N, C) as oc:
        for c in range(C):
            oc.set_cascade(c, SCALES[c], 1.0)
            oc.upload_state(c, (rs.standard_normal((N, N, 2)) * (4e-3 / N)).astype(np.float32))
        oc.set_velocity("on")
        for _ in range(2):
            oc.update(np.float32(1 / 60))
            oc.displace()
        oc.sync()
        s = capi.OceanSet()
        s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, 0.8, 0.5, 1.1
        s.swelldirection[:] = (0.780869, 0.624695)
        s.plane[:] = (0.0, 0.0, 1.0, -0.3)

        hb = torch.from_numpy(bodies.view(np.uint8).reshape(NB, 64).copy()).cuda()
        hm = torch.from_numpy(motions.view(np.uint8).reshape(NB, 32).copy()).cuda()
        db, dm = hb.clone(), hm.clone()
        dq = torch.from_numpy(props.view(np.uint8).reshape(NB, 32).copy()).cuda()
        dp = torch.from_numpy(probes).cuda()
        r0, r1 = (torch.empty(NB * 8, dtype=torch.float32, device="cuda") for _ in range(2))
        r2 = torch.empty(NB * capi.COUPLED_RECORD_FLOATS, dtype=torch.float32, device="cuda")
        dt = float(np.float32(1 / 60))

        def three(cascades, rounds):
            h = float(np.float32(dt) * (np.float32(1) / np.float32(rounds)))
            for _ in range(rounds):
                oc.deposit_body_ripples(cascades, s, db.data_ptr(), dm.data_ptr(), NB, dp.data_ptr(), NB * PER, h, r0.data_ptr(), ITERATIONS)
                oc.step_ripples(h, 1)
                oc.step_bodies(cascades, s, db.data_ptr(), dm.data_ptr(), dq.data_ptr(), NB, dp.data_ptr(), NB * PER, h, 1, r1.data_ptr(), ITERATIONS)

        def coupled(cascades, sub):
            oc.step_bodies_coupled(cascades, s, db.data_ptr(), dm.data_ptr(), dq.data_ptr(), NB, dp.data_ptr(), NB * PER, dt, sub, r2.data_ptr(), ITERATIONS)

        for R, cell in LAYERS:
            oc.set_ripples(R, cell)
            for cascades in ([0], [0, 1, 2, 3]):
                legs = [("(a) deposit + step_ripples + step_bodies", lambda: three(cascades, 1)), ("(b) step_bodies_coupled, substeps 1", lambda: coupled(cascades, 1)),
                        ("(a) x 4", lambda: three(cascades, 4)), ("(c) step_bodies_coupled, substeps 4", lambda: coupled(cascades, 4))]
                times = {label: [] for label, _ in legs}
                for rnd in range(args.rounds + 1):
                    for label, fn in legs:
                        db.copy_(hb)
                        dm.copy_(hm)
                        torch.cuda.synchronize()
                        oc.reset_ripples()
                        oc.sync()
                        t0 = time.perf_counter()
                        for _ in range(args.reps):
                            fn()
                        oc.sync()
                        if rnd:
                            times[label].append((time.perf_counter() - t0) / args.reps * 1e6)
                rec = r2.cpu().numpy().reshape(NB, capi.COUPLED_RECORD_FLOATS)
                print(f"couple_bench {N}^2, R = {R}, list of {len(cascades)}, {NB} bodies x {PER} probes, {ITERATIONS} iterations; "
                      f"{float((rec[:, 6] > 0).mean()):.2f} of the bodies wet, finite records {bool(np.isfinite(rec).all())}, dropped quanta {float(rec[:, 11].sum()):.0f}")
                for label, _ in legs:
                    t = np.array(times[label])
                    print(f"{label:>44}: median {np.median(t):9.1f} us, min {t.min():9.1f} us, max {t.max():9.1f} us per repetition over {len(t)} rounds of {args.reps}")
                a, b = np.array(times[legs[0][0]]), np.array(times[legs[1][0]])
                a4, c4 = np.array(times[legs[2][0]]), np.array(times[legs[3][0]])
                print(f"{'(b) / (a)':>44}: {np.median(b) / np.median(a):.3f} ({b.min() / a.max():.3f} .. {b.max() / a.min():.3f});   "
                      f"(c) / (a) x 4: {np.median(c4) / np.median(a4):.3f} ({c4.min() / a4.max():.3f} .. {c4.max() / a4.min():.3f})")


if __name__ == "__main__":
    main()
