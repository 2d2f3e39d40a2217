"""Drive the surface bounds and the bounded ray cast next to what they are judged against, for one kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o bounds -- python tools/bounds_bench.py
    python tools/bounds_bench.py --split OUT/.../bounds_kernel_trace.csv

On 1024^2 x 4 maps (tools/ray_bench.py's handle and set), `--reps` launches per leg after a warm-up one:
  bounds   displace with the JACOBIAN foam plane (its foam kernel reads the same 16 bytes per point and writes a plane besides), then
           datum_ocean_reduce_bounds: the partial kernel and the final kernel
  casts    tools/ray_bench.py's two ray sets, 10^6 rays each, 4 iterations, (S, R) = (32, 8), with 1 and with 4 cascades, in this order:
           datum_ocean_cast_rays, datum_ocean_cast_rays_bounded, datum_ocean_cast_rays again.  The spread between the plain cast's two
           runs is what the bounded cast is judged against.
Launch order is the order of the legs, so --split cuts the trace's rows per leg."""

import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ray_bench import ALL, C, ITERATIONS, N, ONE, REFINE, SCALES, STEPS, rays_of  # noqa: E402

FOAM, PARTIAL, FINAL, RAYS, BOUNDED = "ocean_foam_kernel", "ocean_bounds_partial_kernel", "ocean_bounds_final_kernel", "ocean_ray_kernel", "ocean_ray_bounded_kernel"
KERNELS = (FOAM, PARTIAL, FINAL, RAYS, BOUNDED)

# (label, kernels of one repetition in launch order, cascade list)
CAST_LEGS = [("rays x1", (RAYS,), ONE), ("bounded x1", (BOUNDED,), ONE), ("rays x1 again", (RAYS,), ONE),
             ("rays x4", (RAYS,), ALL), ("bounded x4", (BOUNDED,), ALL), ("rays x4 again", (RAYS,), ALL)]
SETS = [("random", 10 ** 6), ("fan", 10 ** 6)]


def run(args):
    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)
    with capi.Ocean(N, C) as oc:
        for c in range(C):
            oc.set_cascade(c, SCALES[c], 1.0)
            oc.upload_state(c, (rs.standard_normal((N, N, 2)) * (4e-3 / N)).astype(np.float32))
        oc.set_foam("jacobian")
        for _ in range(args.reps + 1):
            oc.update(np.float32(1 / 60))
            oc.displace()
        oc.sync()
        print(f"bounds_bench foam: {args.reps + 1} displace calls")
        for _ in range(args.reps + 1):
            oc.reduce_bounds()
        oc.sync()
        records = oc.read_bounds()
        print(f"bounds_bench bounds: {args.reps + 2} reduce calls; records\n{records}")
        s = capi.OceanSet()
        s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, 0.8, 0.5, 1.1
        s.swelldirection[:] = (0.780869, 0.624695)
        s.plane[:] = (0.0, 0.0, 1.0, -0.3)
        for cascades in (ONE, ALL):
            print(f"bounds_bench slab of {cascades}: {[float(v) for v in oc.surface_slab(cascades, s)]}")
        for which, n in SETS:
            rays = rays_of(which, n, rs)
            dr = torch.from_numpy(rays).cuda()
            recs = [torch.empty(n * 12, dtype=torch.float32, device="cuda") for _ in range(2)]
            torch.cuda.synchronize()
            oc.sync()
            for label, kernels, cascades in CAST_LEGS:
                bounded = kernels[0] == BOUNDED
                for _ in range(args.reps + 1):
                    (oc.cast_rays_bounded if bounded else oc.cast_rays)(cascades, s, dr.data_ptr(), n, recs[bounded].data_ptr(), ITERATIONS, STEPS, REFINE)
                oc.sync()
                print(f"bounds_bench {which} {n} rays {label}: {args.reps + 1} launches")
                if label.endswith("again"):
                    a, b = (r.cpu().numpy().view(np.uint32) for r in recs)
                    f = recs[0].cpu().numpy()
                    same = bool(np.all((a == b) | np.isnan(f)))
                    status = f.reshape(n, 12)[:, 3]
                    print(f"bounds_bench {which} {n} rays {cascades}: bounded == plain as bits: {same}; miss {np.mean(status == 0):.3f}, "
                          f"enter {np.mean(status == 1):.3f}, leave {np.mean(status == 2):.3f}")
                    assert same


def split(args):
    """per-leg times from the kernel_trace.csv of one run, the warm-up repetition of each leg dropped"""
    rows = []
    with open(args.split) as f:
        for r in csv.DictReader(f):
            for key in KERNELS:
                if key in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), key, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
                    break
    rows = [(key, d) for _, key, d in sorted(rows)]          # launch order, whatever order the trace lists its rows in

    def show(label, d, points=None):
        d = np.asarray(d, np.float64) / 1e3
        extra = f"; {points * 16 / (d.mean() * 1e-6) / 8e12:.3f} of 8 TB/s on 16 B/pt" if points else ""
        print(f"{label:>28}: mean {d.mean():10.2f} us, min {d.min():10.2f} us, max {d.max():10.2f} us over {len(d)} launches{extra}")

    points = N * N * C
    foam = [d for key, d in rows if key == FOAM]
    partial = [d for key, d in rows if key == PARTIAL]
    final = [d for key, d in rows if key == FINAL]
    assert len(foam) == args.reps + 1 and len(partial) == len(final) == args.reps + 2 + 2, (len(foam), len(partial), len(final))
    print(f"{N}^2 x {C}:")
    show("foam JACOBIAN kernel", foam[1:], points)
    show("bounds partial kernel", partial[1:args.reps + 1])
    show("bounds final kernel", final[1:args.reps + 1])
    show("bounds partial + final", np.array(partial[1:args.reps + 1]) + np.array(final[1:args.reps + 1]), points)

    casts = [(key, d) for key, d in rows if key in (RAYS, BOUNDED)]
    assert len(casts) == len(SETS) * len(CAST_LEGS) * (args.reps + 1), len(casts)
    k = 0
    for which, n in SETS:
        print(f"{which}, {n} rays:")
        means = {}
        for label, kernels, _ in CAST_LEGS:
            chunk = casts[k:k + args.reps + 1]
            k += args.reps + 1
            assert all(name == kernels[0] for name, _ in chunk), label
            show(label, [d for _, d in chunk[1:]])
            means[label] = np.mean([d for _, d in chunk[1:]])
        for x in ("x1", "x4"):
            plain = (means[f"rays {x}"], means[f"rays {x} again"])
            print(f"{'bounded / plain ' + x:>28}: {means[f'bounded {x}'] / np.mean(plain):.3f} (the plain cast's two runs: {max(plain) / min(plain):.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--split", help="kernel_trace.csv of a run: print the per-leg times instead of running")
    args = ap.parse_args()
    if args.split:
        split(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
