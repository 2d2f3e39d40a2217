"""Restatements of the ripple layer's bounds (include/datum_ocean_hip.h: datum_ocean_reduce_ripple_bounds) in numpy, beside bounds64.py.

  fold      the layer's record from its state: the extrema as numpy's fmin / fmax reductions (a NaN enters none, an infinity does), both
            counts in integers
  slab32    the rippled slab of a blend list and the layer's record, every line one float32 operation as the header writes it
  slab64    the same lines in float64 from the same float32 records: what the fp32 roundings of the sums are measured against
  eta64     the layer's bilinear height at fp32 points in float64 (ripple64.sample32's patch, wider)

`mistake` plants the errors tests/test_ripple_bounds_emul.py names:
  "no_zero"      the fminf(., 0) / fmaxf(., 0) dropped: the layer's interval no longer holds the 0 a point outside the window reads
  "no_mag"       the layer's term left out of mag: the pad does not cover the layer's roundings
  "min_for_hi"   etamin used for hi
"""

import numpy as np

import ripple64

F = np.float32
RECORD_FLOATS = 8
MISTAKES = ("no_zero", "no_mag", "min_for_hi")


def fold(state):
    """(8,) float32 record of a state [..., 2] (eta, rate), any order of cells"""
    st = np.asarray(state, F).reshape(-1, 2)
    eta, rate = st[:, 0], st[:, 1]
    rec = np.zeros(RECORD_FLOATS, F)
    with np.errstate(invalid="ignore"):
        for k, a in ((0, eta), (2, rate)):
            rec[k] = np.fmin.reduce(a, initial=F(np.inf))
            rec[k + 1] = np.fmax.reduce(a, initial=F(-np.inf))
        rec[4] = F(int((~(np.isfinite(eta) & np.isfinite(rate))).sum()))
        rec[5] = F(int(((eta != 0) | (rate != 0)).sum()))
    return rec


def _slab(T, records, cascades, basez, A, gx, gy, layer, mistake):
    records = np.asarray(records, F).reshape(-1, RECORD_FLOATS)
    layer = np.asarray(layer, F)
    basez, A, gx, gy = (T(F(v)) for v in (basez, A, gx, gy))
    absa = np.abs(A)
    zero = T(0)
    with np.errstate(all="ignore"):
        mag = T(np.abs(basez) + absa)
        hi = T(basez + absa)
        lo = T(basez - absa)
        rx, ry = np.abs(gx), np.abs(gy)
        nonfinite = False
        for c in cascades:
            r = records[int(c)].astype(T)
            mag = T(mag + np.fmax(np.abs(r[0]), np.abs(r[1])))
            hi = T(hi + r[1])
            lo = T(lo + r[0])
            rx = T(rx + np.fmax(np.abs(r[2]), np.abs(r[3])))
            ry = T(ry + np.fmax(np.abs(r[4]), np.abs(r[5])))
            nonfinite = nonfinite or bool(r[6] > 0)
        etamin, etamax = T(layer[0]), T(layer[1])
        elo = etamin if mistake == "no_zero" else np.fmin(etamin, zero)
        ehi = etamax if mistake == "no_zero" else np.fmax(etamax, zero)
        if mistake != "no_mag":
            mag = T(mag + np.fmax(np.abs(elo), np.abs(ehi)))
        hi = T(hi + (elo if mistake == "min_for_hi" else ehi))
        lo = T(lo + elo)
        nonfinite = nonfinite or bool(layer[4] > 0)
        pad = T(mag * T(2.0 ** -16))
        zhi, zlo = T(hi + pad), T(lo - pad)
    if nonfinite:
        zlo = zhi = T(np.nan)
    return zlo, zhi, rx, ry, pad


def slab32(records, cascades, basez, A, gx, gy, layer, mistake=None):
    """(zlo, zhi, reachx, reachy, pad) as float32; records [cascades of the handle][8], layer [8]"""
    out = _slab(F, records, cascades, basez, A, gx, gy, layer, mistake)
    assert all(v.dtype == F for v in out)
    return out


def slab64(records, cascades, basez, A, gx, gy, layer, mistake=None):
    """the same lines in float64"""
    return _slab(np.float64, records, cascades, basez, A, gx, gy, layer, mistake)


def eta64(layer, points):
    """the layer's height at points [n, 2] (rounded to fp32, as a caller hands them over) in float64: the four cells of ripple64.sample32,
    found with its fp32 index arithmetic, the patch in float64; 0 outside the window and beyond 2^30 cells, NaN above a point that is not
    finite"""
    p = np.asarray(points, F).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    R, invs = layer.R, layer.invs
    out = np.zeros(len(p))
    fin = np.isfinite(x) & np.isfinite(y)
    out[~fin] = np.nan
    ok = fin & ripple64._ok(x, invs) & ripple64._ok(y, invs)
    xs, ys = x[ok], y[ok]
    (I0, _), (J0, _) = ripple64._axis(xs, invs), ripple64._axis(ys, invs)
    wx = xs.astype(np.float64) * float(invs) - 0.5 - I0
    wy = ys.astype(np.float64) * float(invs) - 0.5 - J0
    flat = layer.eta.astype(np.float64).reshape(-1)
    c = []
    for k in range(4):
        I, J = I0 + (k & 1), J0 + (k >> 1)
        c.append(np.where(ripple64._inside(I, J, R, layer.ox, layer.oy), flat[ripple64._index(I, J, R)], 0.0))
    e0, e1 = c[0] + wx * (c[1] - c[0]), c[2] + wx * (c[3] - c[2])
    out[ok] = e0 + wy * (e1 - e0)
    return out
