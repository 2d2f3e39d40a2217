"""Wake foam (include/datum_ocean_hip.h: "wake foam") restated, beside ripple64.py and on top of it:

  params            what datum_ocean_step_ripple_foam rounds on the host: hinv = 0.5f invs, the five parameters as fp32, fade;
  update            one update of the plane in MEMORY order, in numpy float32 -- every operation one rounding as written, the bits of
                    datum_amd/csrc/ocean_ripple_foam.h -- or, with dtype=np.float64, the same arithmetic in float64 from the same rounded
                    parameters;
  Plane             the plane as the handle keeps it beside a ripple64.Layer: the torus, step, move (with the layer), reset, window;
  sample32          the bilinear sample.

`mistake` plants the errors tests/test_ripple_foam_emul.py names:
  "no_half"         hinv without the 1/2                         "no_fade"         the old coverage is not faded
  "sum"             g1 + g2 in place of their maximum            "wrap"            neighbours wrap round instead of a zero border
"""

import math

import numpy as np

import ripple64

F = np.float32

MISTAKES = ("no_half", "no_fade", "sum", "wrap")

DEFAULTS = dict(t1=0.04, k1=10.0, t2=0.5, k2=2.0, decay=0.5)

# The fp32 plane against its float64 form after up to three updates from common fp32 states:
#     |f32 - f64| <= K_RFOAM eps (k1 max q + k2 max|eta_t| + 1),        eps = 2^-24, q and eta_t those of the float64 form.
# 3 x the worst distance of THIS restatement from its float64 form over tests/test_ripple_foam_emul.py's cases (measured on the CPU: 0.64,
# at R = 64, origin (37, -11), the default parameters); the device is the restatement bit for bit, so the figure is not taken from the GPU
K_RFOAM = 2.0


def params(invs, dt, t1=0.04, k1=10.0, t2=0.5, k2=2.0, decay=0.5):
    """(hinv, t1, k1, t2, k2, fade) as fp32: fade = (float)exp(-(double)decay (double)dt) from the fp32 decay and dt"""
    fade = F(math.exp(-float(F(decay)) * float(F(dt))))
    return F(0.5) * F(invs), F(t1), F(k1), F(t2), F(k2), fade


def fmax(a, b):
    """fmaxf as ocean_ripple_foam.h decides it: a NaN loses, and of two zeros of opposite sign +0 (their sum)"""
    with np.errstate(all="ignore"):
        return np.where((a == 0) & (b == 0), a + b, np.fmax(a, b))


def update(eta, rate, old, ox, oy, p, dtype=F, mistake=None, parts=False):
    """the plane [R, R] in memory order after one update from the state (eta, rate) [R, R] and the plane `old`"""
    R = eta.shape[0]
    T = dtype
    e, et, old = eta.astype(T), rate.astype(T), old.astype(T)
    hinv, t1, k1, t2, k2, fade = (T(v) for v in p)
    if mistake == "no_half":
        hinv = hinv * T(2)
    wx, wy = ripple64.window_coords(R, ox, oy)
    zero = T(0)
    eL, eR = np.roll(e, 1, 1), np.roll(e, -1, 1)
    eD, eU = np.roll(e, 1, 0), np.roll(e, -1, 0)
    if mistake != "wrap":
        eL = np.where(wx[None, :] == 0, zero, eL)
        eR = np.where(wx[None, :] == R - 1, zero, eR)
        eD = np.where(wy[:, None] == 0, zero, eD)
        eU = np.where(wy[:, None] == R - 1, zero, eU)
    with np.errstate(all="ignore"):
        hx = (eR - eL) * hinv
        hy = (eU - eD) * hinv
        q = hx * hx + hy * hy
        g1 = (q - t1) * k1
        g2 = (np.abs(et) - t2) * k2
        top = g1 + g2 if mistake == "sum" else fmax(g1, g2)
        g = np.fmin(fmax(top, zero), T(1))
        new = fmax(g, old if mistake == "no_fade" else old * fade)
    assert new.dtype == T
    return (new, q, et) if parts else new


def sample32(plane, ox, oy, invs, points):
    """[n] float32 samples of the plane [R, R] (memory order) at points [n, 2]"""
    R = plane.shape[0]
    invs = F(invs)
    p = np.asarray(points, F).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    out = np.zeros(len(p), F)
    fin = np.isfinite(x) & np.isfinite(y)
    out[~fin] = np.nan
    ok = fin & ripple64._ok(x, invs) & ripple64._ok(y, invs)
    (I0, wx), (J0, wy) = ripple64._axis(x[ok], invs), ripple64._axis(y[ok], invs)
    flat = plane.astype(F).reshape(-1)
    f = []
    for k in range(4):
        I, J = I0 + (k & 1), J0 + (k >> 1)
        f.append(np.where(ripple64._inside(I, J, R, ox, oy), flat[ripple64._index(I, J, R)], F(0)).astype(F))
    f0, f1 = f[0] + wx * (f[1] - f[0]), f[2] + wx * (f[3] - f[2])
    res = f0 + wy * (f1 - f0)
    assert res.dtype == F
    out[ok] = res
    return out


class Plane:
    """the plane as the handle keeps it beside `layer` (a ripple64.Layer); dtype float32 (the bits) or float64"""

    def __init__(self, layer, dtype=F, **kw):
        self.layer, self.T = layer, dtype
        self.kw = dict(DEFAULTS, **kw)
        self.f = np.zeros((layer.R, layer.R), dtype)

    def step(self, dt, mistake=None):
        L = self.layer
        self.f = update(L.eta, L.rate, self.f, L.ox, L.oy, params(L.invs, dt, **self.kw), self.T, mistake)

    def move(self, ox, oy):
        """with the layer, BEFORE layer.move: the cells that entered hold no foam"""
        L, m = self.layer, np.arange(self.layer.R)
        world = lambda o: o + ((m - o) & (L.R - 1))
        ent = (world(ox) != world(L.ox))[None, :] | (world(oy) != world(L.oy))[:, None]
        self.f[ent] = 0

    def reset(self):
        self.f[:] = 0

    def window(self):
        return self.layer.window(self.f)

    def sample(self, points):
        L = self.layer
        return sample32(self.f.astype(F), L.ox, L.oy, L.invs, points)
