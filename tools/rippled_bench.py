"""Time the rippled reads next to their parents and next to what a caller paid before them.

    python tools/rippled_bench.py [--reps 20] [--rounds 7]

1024^2 x 4 maps, a ripple layer of R = 1024 cells of 1 m in a non-trivial state, lists of 4 cascades, device arrays only.  Legs:
  mesh   a 1024 x 1024 mesh ("pitched_steep"): gen_blend | gen_blend + sample_ripples over 1024^2 points | gen_blend_rippled -- once with the
         window centred under the mesh's densest vertices ("in view") and once with it 10^5 m away ("outside")
  query  10^6 points, 4 iterations: sample_surface_blend | sample_surface_blend + sample_ripples | sample_surface_blend_rippled
  cast   10^5 rays, 32 steps, 8 bisections: cast_rays | cast_rays_rippled (a caller had no workaround)
The middle leg is what a caller paid before, short of the adding kernel they had to write themselves.  A round enqueues `reps`
repetitions of a leg behind a sync and waits for them: wall-clock per repetition, launch overhead included and overlapped.  One warm-up
round, then `rounds` rounds per leg, the legs interleaved; median and min .. max over the rounds are printed, and the ratios."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, C, MESH, POINTS, RAYS, ITERATIONS, STEPS, REFINE = 1024, 4, 1024, 10 ** 6, 10 ** 5, 4, 32, 8
R, CELL = 1024, 1.0
SCALES = [22.0, 64.0, 9.5, 140.0]
CASCADES = [0, 1, 2, 3]


def measure(oc, legs, reps, rounds):
    import torch

    times = {label: [] for label, _ in legs}
    for rnd in range(rounds + 1):
        for label, fn in legs:
            torch.cuda.synchronize()
            oc.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            oc.sync()
            if rnd:
                times[label].append((time.perf_counter() - t0) / reps * 1e6)
    return {k: np.array(v) for k, v in times.items()}


def show(title, times, parent, paid, rippled, reps):
    print(title)
    for label, t in times.items():
        print(f"{label:>46}: median {np.median(t):9.1f} us, min {t.min():9.1f} us, max {t.max():9.1f} us per repetition over {len(t)} rounds of {reps}")
    r, p = times[rippled], times[parent]
    line = f"{'rippled / parent':>46}: {np.median(r) / np.median(p):.3f} ({r.min() / p.max():.3f} .. {r.max() / p.min():.3f})"
    if paid:
        s = times[paid]
        line += f";   rippled / (parent + sample_ripples): {np.median(r) / np.median(s):.3f} ({r.min() / s.max():.3f} .. {r.max() / s.min():.3f})"
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import torch

    import gen_cases
    from datum_amd import capi
    from oracle import oracle

    rs = np.random.RandomState(1)
    with capi.Ocean(N, C) as oc:
        for c in range(C):
            oc.set_cascade(c, SCALES[c], 1.0)
            oc.upload_state(c, (rs.standard_normal((N, N, 2)) * (4e-3 / N)).astype(np.float32))
        oc.update(np.float32(1 / 60))
        oc.displace()
        oc.sync()

        mesh_set = capi.OceanSet.from_buffer_copy(bytes(gen_cases.oceanset(oracle, N, "pitched_steep", wavescale=SCALES[0])))
        s = capi.OceanSet()
        s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, 0.8, 0.5, 1.1
        s.swelldirection[:] = (0.780869, 0.624695)
        s.plane[:] = (0.0, 0.0, 1.0, -0.3)

        verts = torch.empty(MESH * MESH * 12, dtype=torch.float32, device="cuda")
        oc.gen_blend(CASCADES, mesh_set, MESH, MESH, verts.data_ptr())
        oc.sync()
        v = verts.cpu().numpy().reshape(MESH, MESH, 12)
        gap = np.hypot(*np.moveaxis(np.diff(v[..., :2].astype(np.float64), axis=1), -1, 0))
        near = v[np.unravel_index(np.argmin(gap), gap.shape)][:2]
        mesh_xy = torch.from_numpy(np.ascontiguousarray(v[..., :2].reshape(-1, 2))).cuda()
        mesh_smp = torch.empty(MESH * MESH * 4, dtype=torch.float32, device="cuda")

        def disturb(x, y):
            """the layer centred at (x, y), a few thousand impulses, three sub-steps: a state that is not at rest"""
            oc.set_ripples(0)
            oc.set_ripples(R, CELL)
            oc.center_ripples(float(x), float(y))
            imp = np.zeros((4000, 4), np.float32)
            imp[:, 0] = x + rs.uniform(-0.45, 0.45, 4000) * R * CELL
            imp[:, 1] = y + rs.uniform(-0.45, 0.45, 4000) * R * CELL
            imp[:, 2] = rs.standard_normal(4000) * 0.05
            oc.deposit_ripples_host(imp)
            oc.step_ripples(0.1 * CELL, 3)
            oc.sync()

        for where, (x, y) in (("window in view", near), ("window outside the view", (near[0] + 1.0e5, near[1] + 1.0e5))):
            disturb(x, y)
            legs = [("gen_blend", lambda: oc.gen_blend(CASCADES, mesh_set, MESH, MESH, verts.data_ptr())),
                    ("gen_blend + sample_ripples", lambda: (oc.gen_blend(CASCADES, mesh_set, MESH, MESH, verts.data_ptr()), oc.sample_ripples(mesh_xy.data_ptr(), MESH * MESH, mesh_smp.data_ptr()))),
                    ("gen_blend_rippled", lambda: oc.gen_blend_rippled(CASCADES, mesh_set, MESH, MESH, verts.data_ptr()))]
            t = measure(oc, legs, args.reps, args.rounds)
            oc.sync()
            oc.sample_ripples(mesh_xy.data_ptr(), MESH * MESH, mesh_smp.data_ptr())
            oc.sync()
            share = float((mesh_smp.cpu().numpy().reshape(-1, 4)[:, 0] != 0).mean())
            show(f"rippled_bench mesh {MESH} x {MESH}, {N}^2 x {C}, R = {R}, {where}: {share:.3f} of the vertices over disturbed water", t, "gen_blend", "gen_blend + sample_ripples", "gen_blend_rippled", args.reps)

        disturb(0.0, 0.0)
        pts = torch.from_numpy(rs.uniform(-500, 500, (POINTS, 2)).astype(np.float32)).cuda()
        out = torch.empty(POINTS * 8, dtype=torch.float32, device="cuda")
        smp = torch.empty(POINTS * 4, dtype=torch.float32, device="cuda")
        legs = [("sample_surface_blend", lambda: oc.sample_surface_blend(CASCADES, s, pts.data_ptr(), POINTS, out.data_ptr(), ITERATIONS)),
                ("sample_surface_blend + sample_ripples", lambda: (oc.sample_surface_blend(CASCADES, s, pts.data_ptr(), POINTS, out.data_ptr(), ITERATIONS), oc.sample_ripples(pts.data_ptr(), POINTS, smp.data_ptr()))),
                ("sample_surface_blend_rippled", lambda: oc.sample_surface_blend_rippled(CASCADES, s, pts.data_ptr(), POINTS, out.data_ptr(), ITERATIONS))]
        t = measure(oc, legs, args.reps, args.rounds)
        show(f"rippled_bench query {POINTS} points, {ITERATIONS} iterations, list of {len(CASCADES)}", t, "sample_surface_blend", "sample_surface_blend + sample_ripples", "sample_surface_blend_rippled", args.reps)

        rays = np.zeros((RAYS, 8), np.float32)
        rays[:, 0:2] = rs.uniform(-480, 480, (RAYS, 2))
        rays[:, 2] = 0.3 + rs.uniform(2.5, 4.0, RAYS)
        d = rs.standard_normal((RAYS, 3))
        d[:, 2] = -np.abs(d[:, 2]) - 0.1
        rays[:, 4:7] = d
        rays[:, 7] = 8.0 / np.abs(d[:, 2])
        dr = torch.from_numpy(rays).cuda()
        rec = torch.empty(RAYS * 12, dtype=torch.float32, device="cuda")
        legs = [("cast_rays", lambda: oc.cast_rays(CASCADES, s, dr.data_ptr(), RAYS, rec.data_ptr(), ITERATIONS, STEPS, REFINE)),
                ("cast_rays_rippled", lambda: oc.cast_rays_rippled(CASCADES, s, dr.data_ptr(), RAYS, rec.data_ptr(), ITERATIONS, STEPS, REFINE))]
        t = measure(oc, legs, args.reps, args.rounds)
        hits = float((rec.cpu().numpy().reshape(-1, 12)[:, 3] > 0).mean())
        show(f"rippled_bench cast {RAYS} rays, {STEPS} steps, {REFINE} bisections, {ITERATIONS} iterations, list of {len(CASCADES)}: {hits:.2f} hit", t, "cast_rays", None, "cast_rays_rippled", args.reps)


if __name__ == "__main__":
    main()
