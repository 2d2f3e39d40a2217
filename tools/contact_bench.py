"""Time body contact next to coupled stepping.

    python tools/contact_bench.py [--reps 10] [--rounds 7]

4096 bodies x 64 probes on 1024^2 maps, lists of 1 and of 4 cascades, 4 iterations, device arrays only; a ripple layer of 1024^2 cells of
1 m with a bed (a 64 x 64 map, 5 m deep) and 16 or 256 walls (boxes of 2 m in a corner of the window that no body reaches).  One
sub-step per call.  Three legs per list and wall count:
  (a) datum_ocean_step_bodies_coupled                                        the parent's call, the same kernel as before
  (b) datum_ocean_step_bodies_contact, flags BED | WALLS, nothing touching   every probe walks the bed's patch and the whole wall list
  (c) datum_ocean_step_bodies_contact, flags BED | WALLS, every body grounded (hulls without buoyancy set down 0.2 m into the bed)
A round enqueues `reps` repetitions of a leg behind a sync and waits for them: wall-clock per repetition, launch overhead and the layer's
own sub-step included (it is the same in all three legs).  One warm-up round, then `rounds` rounds per leg, the legs interleaved; median
and min .. max over the rounds are printed.  Bodies and the layer are reset before every round so that each leg sees the same poses."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C, NB, PER, ITERATIONS, R, CELL, DEPTH = 1024, 4, 4096, 64, 4, 1024, 1.0, 5.0
SCALES = (22.0, 67.0, 211.0, 677.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)
    bodies = np.zeros(NB, capi.BODY_DTYPE)
    bodies["rotation"] = np.eye(3, dtype=np.float32).ravel()
    bodies["position"] = np.stack([rs.uniform(-480, 480, NB), rs.uniform(-480, 480, NB), rs.uniform(-0.5, 0.2, NB)], 1)
    bodies["first"], bodies["count"], bodies["cap"] = np.arange(NB) * PER, PER, 1.0
    grounded = bodies.copy()
    grounded["position"][:, 2] = -DEPTH - 0.2
    motions = np.zeros(NB, capi.BODY_MOTION_DTYPE)
    motions["linear"], motions["angular"] = rs.uniform(-1, 1, (NB, 3)), rs.uniform(-0.2, 0.2, (NB, 3))
    motions["cl"], motions["cq"] = 500.0, 200.0
    props = np.zeros(NB, capi.BODY_PROPS_DTYPE)
    props["invmass"], props["invinertia"], props["gravity"], props["buoyancy"] = 1 / 4000.0, 1 / 3000.0, 9.81, 9810.0
    heavy = props.copy()
    heavy["buoyancy"] = 0.0
    probes = np.zeros((NB * PER, 4), np.float32)
    g = np.linspace(-1.5, 1.5, 8)
    xx, yy = np.meshgrid(g, g)
    probes[:, 0], probes[:, 1], probes[:, 3] = np.tile(xx.ravel(), NB), np.tile(yy.ravel(), NB), 9.0 / PER

    bed = np.zeros(1, capi.RIPPLE_BED)
    bed["width"], bed["height"], bed["origin"], bed["texel"], bed["outside"] = 64, 64, (-520.0, -520.0), 16.5, DEPTH
    bed["max_depth"], bed["dry_depth"], bed["surf_depth"], bed["surf_gamma"] = DEPTH, 0.05, 0.0, 0.0
    depths = np.full((64, 64), DEPTH, np.float32)
    contact = capi.BodyContact(2.0e4, 400.0, 60.0, capi.CONTACT_BED | capi.CONTACT_WALLS)

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
        hg = torch.from_numpy(grounded.view(np.uint8).reshape(NB, 64).copy()).cuda()
        hm = torch.from_numpy(motions.view(np.uint8).reshape(NB, 32).copy()).cuda()
        db, dm = hb.clone(), hm.clone()
        dq = torch.from_numpy(props.view(np.uint8).reshape(NB, 32).copy()).cuda()
        dh = torch.from_numpy(heavy.view(np.uint8).reshape(NB, 32).copy()).cuda()
        dp = torch.from_numpy(probes).cuda()
        rec = torch.empty(NB * 16, dtype=torch.float32, device="cuda")
        dt = float(np.float32(1 / 60))

        oc.set_ripples(R, CELL)
        oc.set_ripple_bed(bed[0], depths)

        for nwalls in (16, 256):
            walls = np.zeros(nwalls, capi.RIPPLE_WALL)
            k = np.arange(nwalls)
            walls["center"] = np.stack([490.0 + 3.0 * (k % 6), 490.0 - 3.0 * (k // 6)], 1)
            walls["axis"], walls["half"], walls["kind"] = (1.0, 0.0), (1.0, 1.0), k % 2
            oc.set_ripple_walls(walls)
            for cascades in ([0], [0, 1, 2, 3]):
                args_ = lambda q=dq: (cascades, s, db.data_ptr(), dm.data_ptr(), q.data_ptr(), NB, dp.data_ptr(), NB * PER, dt, 1, rec.data_ptr())
                legs = [("(a) step_bodies_coupled", hb, lambda: oc.step_bodies_coupled(*args_(), ITERATIONS)),
                        ("(b) step_bodies_contact, nothing touching", hb, lambda: oc.step_bodies_contact(*args_(), contact, ITERATIONS)),
                        ("(c) step_bodies_contact, all grounded", hg, lambda: oc.step_bodies_contact(*args_(dh), contact, ITERATIONS))]
                times = {label: [] for label, _, _ in legs}
                touched = {}
                for rnd in range(args.rounds + 1):
                    for label, start, fn in legs:
                        oc.reset_ripples()
                        db.copy_(start)
                        dm.copy_(hm)
                        torch.cuda.synchronize()
                        oc.sync()
                        t0 = time.perf_counter()
                        for _ in range(args.reps):
                            fn()
                        oc.sync()
                        if rnd:
                            times[label].append((time.perf_counter() - t0) / args.reps * 1e6)
                        if label[1] != "a":
                            r = rec.cpu().numpy().reshape(NB, 16)
                            touched[label] = (float((r[:, 15] > 0).mean()), bool(np.isfinite(r).all()))
                print(f"contact_bench {N}^2, list of {len(cascades)}, {NB} bodies x {PER} probes, {ITERATIONS} iterations, layer {R}^2, {nwalls} walls; "
                      + "; ".join(f"{label[:3]} touching {t:.2f} finite {f}" for label, (t, f) in touched.items()))
                for label, _, _ in legs:
                    t = np.array(times[label])
                    print(f"{label:>44}: median {np.median(t):9.1f} us, min {t.min():9.1f} us, max {t.max():9.1f} us per repetition over {len(t)} rounds of {args.reps}")


if __name__ == "__main__":
    main()
