"""Restatements of the surface bounds (include/datum_ocean_hip.h: datum_ocean_reduce_bounds) in numpy.

  fold      a cascade's record from its texels: the extrema as numpy's fmin / fmax reductions (a NaN enters none, an infinity does: nanmin /
            nanmax with +inf / -inf for "no value"), nonfinite counted in integers
  slab32    the slab of a blend list, every line one float32 operation as the header writes it
  frame32   basez, |A|'s A and the Gerstner terms gx, gy as the module's host code forms them in float32 (ocean_gen.hip: make_gen_frame)
"""

import numpy as np

F = np.float32
RECORD_FLOATS = 8


def fold(dx, dy, dz):
    """(8,) float32 record of the texels' (dx, dy, dz), any shape"""
    dx, dy, dz = (np.asarray(a, F).ravel() for a in (dx, dy, dz))
    rec = np.zeros(RECORD_FLOATS, F)
    with np.errstate(invalid="ignore"):
        for k, a in ((0, dz), (2, dx), (4, dy)):
            rec[k] = np.fmin.reduce(a, initial=F(np.inf))
            rec[k + 1] = np.fmax.reduce(a, initial=F(-np.inf))
    rec[6] = F(int((~(np.isfinite(dx) & np.isfinite(dy) & np.isfinite(dz))).sum()))
    return rec


def fold_maps(maps):
    """the record of a logical map image [2][N][N][4] (read_maps): layer 0's x, y, z"""
    m = np.asarray(maps, F)[0]
    return fold(m[..., 0], m[..., 1], m[..., 2])


def frame32(s):
    """(basez, A, gx, gy) in float32 from a datum_ocean_set"""
    A = F(s.swellamplitude)
    frequency = F(2 * 3.14159265358979323846) / F(s.swelllength)
    with np.errstate(all="ignore"):
        qi = F(s.swellsteepness) / (frequency * A * F(4) + F(1e-6))
        gx = qi * A * F(s.swelldirection[0])
        gy = qi * A * F(s.swelldirection[1])
    return -F(s.plane[3]), A, gx, gy


def slab32(records, cascades, basez, A, gx, gy):
    """(zlo, zhi, reachx, reachy, pad) as float32; records [cascades of the handle][8]"""
    records = np.asarray(records, F).reshape(-1, RECORD_FLOATS)
    basez, A, gx, gy = F(basez), F(A), F(gx), F(gy)
    absa = np.abs(A)
    with np.errstate(all="ignore"):
        mag = np.abs(basez) + absa
        hi = basez + absa
        lo = basez - absa
        rx, ry = np.abs(gx), np.abs(gy)
        nonfinite = False
        for c in cascades:
            r = records[int(c)]
            mag = F(mag + np.fmax(np.abs(r[0]), np.abs(r[1])))
            hi = F(hi + r[1])
            lo = F(lo + r[0])
            rx = F(rx + np.fmax(np.abs(r[2]), np.abs(r[3])))
            ry = F(ry + np.fmax(np.abs(r[4]), np.abs(r[5])))
            nonfinite = nonfinite or bool(r[6] > 0)
        pad = F(mag * F(2.0 ** -16))
        zhi, zlo = F(hi + pad), F(lo - pad)
    if nonfinite:
        zlo = zhi = F(np.nan)
    return zlo, zhi, rx, ry, pad
