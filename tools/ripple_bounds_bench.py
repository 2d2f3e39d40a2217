"""Drive the ripple layer's bounds and the bounded rippled cast next to what they are judged against, for one kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o ripple_bounds -- python tools/ripple_bounds_bench.py
    python tools/ripple_bounds_bench.py --split OUT/.../ripple_bounds_kernel_trace.csv

On 1024^2 x 4 maps (tools/ray_bench.py's handle and set) and a ripple layer of 1 m cells in a non-trivial state, `--reps` repetitions per leg
after a warm-up one:
  bounds   at R = 256 and at R = 1024: datum_ocean_step_ripples with two sub-steps -- the second is ocean_ripple_step_kernel<false>, which
           reads and writes the state the reduction only reads -- then datum_ocean_reduce_ripple_bounds: the partial and the final kernel
  casts    R = 1024; tools/ray_bench.py's two ray sets and a set wholly inside the rippled slab, 10^6 rays each, 4 iterations,
           (S, R) = (32, 8), with 1 and with 4 cascades, in this order: datum_ocean_cast_rays_rippled, datum_ocean_cast_rays_rippled_bounded,
           datum_ocean_cast_rays_rippled again.  The spread between the rippled cast's two runs is what the bounded one is judged against.
Records are compared as bits in the run.  Launch order is the order of the legs, so --split cuts the trace's rows per leg."""

import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ray_bench import ALL, C, ITERATIONS, N, ONE, REFINE, SCALES, STEPS, rays_of  # noqa: E402

STEP, PARTIAL, FINAL = "ocean_ripple_step_kernel", "ocean_ripple_bounds_partial_kernel", "ocean_ripple_bounds_final_kernel"
RIPPLED, BOUNDED = "ocean_ray_rippled_kernel", "ocean_ray_rippled_bounded_kernel"
KERNELS = (STEP, PARTIAL, FINAL, RIPPLED, BOUNDED)

SIZES = (256, 1024)
CELL = 1.0

# (label, kernel of one repetition, cascade list)
CAST_LEGS = [("rippled x1", RIPPLED, ONE), ("bounded x1", BOUNDED, ONE), ("rippled x1 again", RIPPLED, ONE),
             ("rippled x4", RIPPLED, ALL), ("bounded x4", BOUNDED, ALL), ("rippled x4 again", RIPPLED, ALL)]
SETS = [("random", 10 ** 6), ("fan", 10 ** 6), ("inside", 10 ** 6)]


def inside_rays(n, rs, zlo, zhi):
    """segments over and beside the window whose two ends lie in the slab's middle four fifths: no sample is decided by the slab"""
    r = np.zeros((n, 8), np.float32)
    lo, hi = 0.9 * zlo + 0.1 * zhi, 0.1 * zlo + 0.9 * zhi
    z0, z1 = rs.uniform(lo, hi, n), rs.uniform(lo, hi, n)
    az, run = rs.uniform(0, 2 * np.pi, n), rs.uniform(1, 60, n)
    r[:, 0:2] = rs.uniform(-1000, 1000, (n, 2))
    r[:, 2] = z0
    r[:, 4], r[:, 5], r[:, 6] = run * np.cos(az), run * np.sin(az), z1 - z0
    r[:, 3], r[:, 7] = 0.0, 1.0
    return r


def run(args):
    import torch

    from datum_amd import capi

    rs = np.random.RandomState(1)
    with capi.Ocean(N, C) as oc:
        for c in range(C):
            oc.set_cascade(c, SCALES[c], 1.0)
            oc.upload_state(c, (rs.standard_normal((N, N, 2)) * (4e-3 / N)).astype(np.float32))
        oc.update(np.float32(1 / 60))
        oc.displace()
        oc.reduce_bounds()
        oc.sync()

        def disturb(R):
            """the layer centred at the origin, a few thousand impulses, three sub-steps: a state that is not at rest"""
            oc.set_ripples(0)
            oc.set_ripples(R, CELL)
            imp = np.zeros((4000, 4), np.float32)
            imp[:, 0:2] = rs.uniform(-0.45, 0.45, (4000, 2)) * R * CELL
            imp[:, 2] = rs.standard_normal(4000) * 0.05
            oc.deposit_ripples_host(imp)
            oc.step_ripples(0.1 * CELL, 3)
            oc.sync()

        for R in SIZES:
            disturb(R)
            for _ in range(args.reps + 1):
                oc.step_ripples(0.05 * CELL, 2)
            oc.sync()
            for _ in range(args.reps + 1):
                oc.reduce_ripple_bounds()
            oc.sync()
            print(f"ripple_bounds_bench R = {R}: {args.reps + 1} steps of two sub-steps, {args.reps + 1} reduce calls; record {oc.read_ripple_bounds().tolist()}")

        # (R = 1024 from here on; the read above reduced once more, and the record is current)
        s = capi.OceanSet()
        s.swelllength, s.swellamplitude, s.swellsteepness, s.swellphase = 40.0, 0.8, 0.5, 1.1
        s.swelldirection[:] = (0.780869, 0.624695)
        s.plane[:] = (0.0, 0.0, 1.0, -0.3)
        slabs = {}
        for cascades in (ONE, ALL):
            slabs[len(cascades)] = [float(v) for v in oc.surface_slab_rippled(cascades, s)]
            print(f"ripple_bounds_bench rippled slab of {cascades}: {slabs[len(cascades)]}; un-rippled: {[float(v) for v in oc.surface_slab(cascades, s)]}")
        for which, n in SETS:
            # (inside the narrower of the two slabs, the single cascade's: inside both)
            rays = inside_rays(n, rs, slabs[1][0], slabs[1][1]) if which == "inside" else rays_of(which, n, rs)
            dr = torch.from_numpy(rays).cuda()
            recs = [torch.empty(n * 12, dtype=torch.float32, device="cuda") for _ in range(2)]
            torch.cuda.synchronize()
            oc.sync()
            for label, kernel, cascades in CAST_LEGS:
                bounded = kernel == BOUNDED
                for _ in range(args.reps + 1):
                    (oc.cast_rays_rippled_bounded if bounded else oc.cast_rays_rippled)(cascades, s, dr.data_ptr(), n, recs[bounded].data_ptr(), ITERATIONS, STEPS, REFINE)
                oc.sync()
                print(f"ripple_bounds_bench {which} {n} rays {label}: {args.reps + 1} launches")
                if label.endswith("again"):
                    a, b = (r.cpu().numpy().view(np.uint32) for r in recs)
                    f = recs[0].cpu().numpy()
                    same = bool(np.all((a == b) | np.isnan(f)))
                    status = f.reshape(n, 12)[:, 3]
                    print(f"ripple_bounds_bench {which} {n} rays {cascades}: bounded == rippled as bits: {same}; miss {np.mean(status == 0):.3f}, "
                          f"enter {np.mean(status == 1):.3f}, leave {np.mean(status == 2):.3f}")
                    assert same


def split(args):
    """per-leg times from the kernel_trace.csv of one run, the warm-up repetition of each leg dropped"""
    rows = []
    with open(args.split) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            for key in KERNELS:
                if key in name:
                    if key == STEP:
                        key = STEP + ("<false>" if ("<false>" in name or "ILb0E" in name) else "<true>")
                    rows.append((int(r["Start_Timestamp"]), key, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
                    break
    rows = [(key, d) for _, key, d in sorted(rows)]          # launch order, whatever order the trace lists its rows in

    def show(label, d, bytes_=None):
        d = np.asarray(d, np.float64) / 1e3
        extra = f"; {bytes_ / (d.mean() * 1e-6) / 8e12:.3f} of 8 TB/s on {bytes_ / 2 ** 20:.1f} MiB" if bytes_ else ""
        print(f"{label:>34}: mean {d.mean():10.2f} us, min {d.min():10.2f} us, max {d.max():10.2f} us over {len(d)} launches{extra}")
        return d.mean()

    reps = args.reps
    steps = [d for key, d in rows if key == STEP + "<false>"]
    partial = [d for key, d in rows if key == PARTIAL]
    final = [d for key, d in rows if key == FINAL]
    # per size: disturb's three sub-steps give two <false> launches, then reps + 1 steps of one each; reps + 1 reduces and the read's one.
    # The slab calls behind the sizes reduce twice more at the last size
    per_step, per_reduce = 2 + reps + 1, reps + 2
    assert len(steps) == len(SIZES) * per_step and len(partial) == len(final) == len(SIZES) * per_reduce + 2, (len(steps), len(partial), len(final))
    for k, R in enumerate(SIZES):
        print(f"R = {R}:")
        st = steps[k * per_step + 3:(k + 1) * per_step]
        pa = partial[k * per_reduce + 1:k * per_reduce + 1 + reps]
        fi = final[k * per_reduce + 1:k * per_reduce + 1 + reps]
        a = show("ripple step kernel<false>", st, R * R * 16)
        show("ripple bounds partial kernel", pa, R * R * 8)
        show("ripple bounds final kernel", fi)
        b = show("ripple bounds partial + final", np.array(pa) + np.array(fi), R * R * 8)
        print(f"{'(partial + final) / step<false>':>34}: {b / a:.3f}")

    casts = [(key, d) for key, d in rows if key in (RIPPLED, BOUNDED)]
    assert len(casts) == len(SETS) * len(CAST_LEGS) * (reps + 1), len(casts)
    k = 0
    for which, n in SETS:
        print(f"{which}, {n} rays:")
        means = {}
        for label, kernel, _ in CAST_LEGS:
            chunk = casts[k:k + reps + 1]
            k += reps + 1
            assert all(name == kernel for name, _ in chunk), label
            means[label] = show(label, [d for _, d in chunk[1:]])
        for x in ("x1", "x4"):
            plain = (means[f"rippled {x}"], means[f"rippled {x} again"])
            ratio, spread = means[f"bounded {x}"] / np.mean(plain), max(plain) / min(plain)
            verdict = "not slower than the rippled cast beyond its own spread" if means[f"bounded {x}"] <= max(plain) * spread else "SLOWER than the rippled cast beyond its own spread"
            print(f"{'bounded / rippled ' + x:>34}: {ratio:.3f} (the rippled cast's two runs: {spread:.3f}): {verdict}")


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
