"""The wake half-angle of a moving point source under the ripple layer's DEEP step, in the float64 model.  No GPU.

    python tools/ripple_deep_wake_angle.py [--R 256] [--cell 0.25] [--h 0.05] [--speeds 2 4]

tests/ripple_deep64.py's Layer in float64 (gamma = 0, a sponge of 16 cells), g = 9.81.  The source starts 24 m behind the window's middle,
moves along +x for 44 m and deposits 0.0625 m^3 per sub-step where it stands.  Estimator: in each column 8 .. 30 m behind the source, in
steps of 1 m, the angle, seen from the source, of the cell with the largest |eta| (cells further out than 0.9 x the distance astern or than
28 m are not looked at); the median and the quartiles over the 22 columns are printed.  The largest crest lies INSIDE the caustic, so the
estimator reads below the wedge's 19.47 degrees even for exact deep water.  A number for the documents, not a test."""

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

G = 9.81


def half_angle(R, cell, h, U):
    import ripple_deep64 as rd

    lay = rd.Layer(R, cell, np.float64, gamma=0.0, B=16, sponge_gamma=4.0)
    assert rd.stable(lay.g, cell, h, 1, lay.G)
    x0 = -24.0
    n = int(44.0 / U / h)
    for k in range(n):
        lay.deposit(np.array([[x0 + U * k * h, 0.0, 0.0625, 0.0]], np.float32))
        lay.step(h, 1)
    xs = x0 + U * n * h
    eta = lay.window()[..., 0]
    c = (np.arange(R) + lay.ox + 0.5) * cell
    angles = []
    for d in np.arange(8.0, 30.0, 1.0):
        i = int(np.argmin(np.abs(c - (xs - d))))
        seen = (np.abs(c) < 0.9 * d) & (np.abs(c) < 28)
        j = int(np.argmax(np.where(seen, np.abs(eta[:, i]), 0)))
        angles.append(np.degrees(np.arctan2(abs(c[j]), d)))
    return np.array(angles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=256)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--h", type=float, default=0.05)
    ap.add_argument("--speeds", type=float, nargs="+", default=[2.0, 4.0])
    args = ap.parse_args()

    for U in args.speeds:
        a = half_angle(args.R, args.cell, args.h, U)
        lam = 2 * np.pi * U * U / G
        print(f"U = {U} m/s: half-angle of the largest |eta| per column 8..30 m behind the source: median {np.median(a):.1f} deg, quartiles "
              f"{np.percentile(a, 25):.1f} .. {np.percentile(a, 75):.1f} deg (Kelvin 19.47; transverse wavelength 2 pi U^2 / g = {lam:.1f} m = {lam / args.cell:.0f} cells)", flush=True)


if __name__ == "__main__":
    main()
