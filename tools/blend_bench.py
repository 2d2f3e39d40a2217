"""Drive the several-cascade calls next to the single-cascade ones for one kernel trace.

    rocprofv3 --kernel-trace --stats -d OUT -o blend -- python tools/blend_bench.py
    python tools/blend_bench.py --split OUT/.../blend_kernel_trace.csv

On 1024^2 x 4 maps (wavescales 22, 64, 9.5, 140), `--reps` launches per leg after a warm-up launch, in this order:
  mesh of 1024 x 1024      datum_ocean_gen (cascade 0), then datum_ocean_gen_blend with 1, 2 and 4 cascades; the single leg once more at the
                           end: the spread between the two single legs is what the 1-cascade leg is judged against
  10^6 points, 4 iterations  datum_ocean_sample_surface, then the blend with 1 and 4 cascades, then the single leg again
Launch order is the order of the legs, so --split cuts the trace's rows per leg."""

import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, C, MESH, POINTS, ITERATIONS = 1024, 4, 1024, 10 ** 6, 4
SCALES = [22.0, 64.0, 9.5, 140.0]

# (label, kernel name in the trace, cascade list; None: the single-cascade call on cascade 0)
MESH_LEGS = [("gen", "ocean_gen_kernel", None), ("gen_blend x1", "ocean_gen_blend_kernel", [0]), ("gen_blend x2", "ocean_gen_blend_kernel", [0, 1]),
             ("gen_blend x4", "ocean_gen_blend_kernel", [0, 1, 2, 3]), ("gen again", "ocean_gen_kernel", None)]
QUERY_LEGS = [("surface", "ocean_surface_kernel", None), ("surface_blend x1", "ocean_surface_blend_kernel", [0]),
              ("surface_blend x4", "ocean_surface_blend_kernel", [0, 1, 2, 3]), ("surface again", "ocean_surface_kernel", None)]


def run(args):
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
        s = capi.OceanSet.from_buffer_copy(bytes(gen_cases.oceanset(oracle, N, "pitched_steep", wavescale=SCALES[0])))
        s.scale = np.float32(1.0) / np.float32(SCALES[0])
        verts = torch.empty(MESH * MESH * 12, dtype=torch.float32, device="cuda")
        pts = torch.from_numpy(rs.uniform(-1000, 1000, (POINTS, 2)).astype(np.float32)).cuda()
        out = torch.empty(POINTS * 8, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        oc.sync()
        for label, _, cascades in MESH_LEGS:
            for _ in range(args.reps + 1):
                if cascades is None:
                    oc.gen(0, s, MESH, MESH, verts.data_ptr())
                else:
                    oc.gen_blend(cascades, s, MESH, MESH, verts.data_ptr())
            oc.sync()
            print(f"blend_bench mesh {MESH}x{MESH} {label}: {args.reps + 1} launches")
        for label, _, cascades in QUERY_LEGS:
            for _ in range(args.reps + 1):
                if cascades is None:
                    oc.sample_surface(0, s, pts.data_ptr(), POINTS, out.data_ptr(), ITERATIONS)
                else:
                    oc.sample_surface_blend(cascades, s, pts.data_ptr(), POINTS, out.data_ptr(), ITERATIONS)
            oc.sync()
            print(f"blend_bench query {POINTS} points {label}: {args.reps + 1} launches")


def split(args):
    """per-leg mean kernel time from the kernel_trace.csv of one run (the warm-up launch of each leg dropped)"""
    rows = []
    with open(args.split) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            for key in ("ocean_gen_blend_kernel", "ocean_surface_blend_kernel", "ocean_gen_kernel", "ocean_surface_kernel"):
                if key in name:
                    rows.append((int(r["Start_Timestamp"]), key, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
                    break
    rows = [(key, d) for _, key, d in sorted(rows)]          # launch order, whatever order the trace lists its rows in
    per = args.reps + 1
    legs = MESH_LEGS + QUERY_LEGS
    assert len(rows) == per * len(legs), (len(rows), per * len(legs))
    for k, (label, kernel, _) in enumerate(legs):
        chunk = rows[k * per:(k + 1) * per]
        assert all(name == kernel for name, _ in chunk), (label, kernel)
        d = np.array([t for _, t in chunk[1:]], np.float64) / 1e3
        print(f"{label:>18}: mean {d.mean():8.2f} us, min {d.min():8.2f} us, max {d.max():8.2f} us over {len(d)} launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--split", help="kernel_trace.csv of a run: print the per-leg kernel means instead of running")
    args = ap.parse_args()
    if args.split:
        split(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
