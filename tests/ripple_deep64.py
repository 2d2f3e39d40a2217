"""The ripple layer's DEEP step (include/datum_ocean_hip.h: "dispersive ripples") restated, beside ripple64.py and on top of it:

  weights64         the quadrant table G0[l][k] by the definition, in float64, the mean of the 169 unfolded weights already taken off;
  weights32         the 49 fp32 weights: weights64 rounded, the centre corrected so that the 169 sum to the smallest value >= 0;
  symbol            G^(theta) = sum F(di, dj) cos(di theta_x) cos(dj theta_y) on a grid of theta;
  params            what a DEEP step rounds on the host: h, gs = g / s and the sponge table f[0 .. B];
  stable            what the call accepts: h sqrt(g sum|F| / s) <= 1.9, in double from the fp32 weights;
  substep           one sub-step over the layer in MEMORY order, in numpy float32 -- every operation one rounding as written, the bits of
                    datum_amd/csrc/ocean_ripple_deep.h -- or, with dtype=np.float64, the same arithmetic in float64 from the same rounded
                    parameters; `periodic` (TEST ONLY: no call has it) lets the stencil wrap round the torus instead of reading 0 outside;
  Layer             ripple64.Layer with the mode: WAVE steps as its parent, DEEP with substep above.

`mistake` plants the errors tests/test_ripple_deep64.py names:
  "swap"            G[|di|][|dj|] for G[|dj|][|di|] (shows with an asymmetric probe table only: the real one is symmetric)
  "sign"            the rate moves WITH acc                        "gs_product"  g * s for g / s
  "centre"          the centre weight is not corrected (weights32)
"""

import functools

import numpy as np

import ripple64

F = np.float32
P = 6
Q = P + 1
M = 1024
WAVE, DEEP = 0, 1
G_DEFAULT = float(F(9.81))

MISTAKES = ("swap", "sign", "gs_product", "centre")

# The device against float64, for one DEEP datum_ocean_step_ripples call (up to 16 sub-steps) from a common fp32 state:
# |eta - eta64| <= K_RIP_DEEP eps max|eta64|.  3 x the worst distance of THIS restatement from its float64 form over
# tests/test_ripple_deep_emul.py's cases (measured on the CPU: 14.52, at R = 64, origin (0, 0), 16 sub-steps, B = 8); the device is the
# restatement bit for bit, so the figure is not taken from the GPU
K_RIP_DEEP = 43.6

FOLD = np.array([1.0] + [2.0] * P)


@functools.lru_cache(maxsize=None)
def _weights64():
    theta = 2.0 * np.pi * (np.arange(M) - M // 2) / M
    C = np.cos(np.arange(Q)[:, None] * theta[None, :])                     # [k][a]
    cone = np.sqrt(theta[:, None] ** 2 + theta[None, :] ** 2)              # [b][a]
    G0 = (C @ cone @ C.T) / float(M * M)                                   # [l][k] = sum_b sum_a cos(l theta_b) cone[b][a] cos(k theta_a)
    total = float((FOLD[:, None] * FOLD[None, :] * G0).sum())
    return G0 - total / 169.0


def weights64():
    """[7, 7] float64, [l][k]: the definition's steps 1 and 2 short of the rounding"""
    return _weights64().copy()


def unfold(G):
    """[13, 13]: F[dj + 6][di + 6] = G[|dj|][|di|]"""
    i = np.abs(np.arange(-P, P + 1))
    return np.asarray(G)[np.ix_(i, i)]


def weights32(mistake=None):
    """[7, 7] float32, [l][k]: step 2's rounding and step 3's centre"""
    G = weights64().astype(F)
    if mistake == "centre":
        return G
    Fd = unfold(G).astype(np.float64)
    rest = float(Fd.sum() - Fd[P, P])
    c = F(-rest)
    if rest + float(c) < 0.0:
        c = np.nextafter(c, F(np.inf))
    G[0, 0] = c
    return G


def mass(G):
    """sum |F| over the 169 weights, in double"""
    return float(np.abs(unfold(G).astype(np.float64)).sum())


def symbol(G, n, swap=False):
    """G^ on the n x n grid theta = 2 pi (a - n/2) / n: ([n, n] indexed [y][x], theta [n])"""
    theta = 2.0 * np.pi * (np.arange(n) - n // 2) / n
    C = FOLD[:, None] * np.cos(np.arange(Q)[:, None] * theta[None, :])     # [k][a]
    G = np.asarray(G, np.float64)
    return C.T @ (G.T if swap else G) @ C, theta


def symbol_at(G, tx, ty):
    G = np.asarray(G, np.float64)
    cx, cy = FOLD * np.cos(np.arange(Q) * tx), FOLD * np.cos(np.arange(Q) * ty)
    return float(cy @ G @ cx)


def params(g, s, gamma, B, sponge_gamma, dt, substeps, mistake=None):
    """(h, gs, f): h = dt * (1 / substeps) in fp32; gs and f[0 .. B] in double from the fp32 g, s, gamma, sponge_gamma, rounded once"""
    h, _, f = ripple64.params(1.0, s, gamma, B, sponge_gamma, dt, substeps)
    g, s = float(F(g)), float(F(s))
    return h, F(g * s if mistake == "gs_product" else g / s), f


def bound(g, s, dt, substeps, G):
    h = F(dt) * (F(1) / F(substeps))
    return float(h) * np.sqrt(float(F(g)) * mass(G) / float(F(s)))


def stable(g, s, dt, substeps, G):
    h = F(dt) * (F(1) / F(substeps))
    return float(h) >= 0 and bound(g, s, dt, substeps, G) <= 1.9


def substep(eta, rate, src, ox, oy, B, h, gs, f, G, first, dtype=F, mistake=None, periodic=False):
    """(eta, rate) [R, R] in memory order after one DEEP sub-step; src [R, R] int32 is read by a step's first sub-step only"""
    R = eta.shape[0]
    T = dtype
    eta, rate = eta.astype(T), rate.astype(T)
    h, gs, f = T(h), T(gs), np.asarray(f).astype(T)
    G = np.asarray(G, F).astype(T)
    e = eta + src.astype(T) * T(ripple64.UNIT) if first else eta
    wx, wy = ripple64.window_coords(R, ox, oy)
    zero = T(0)
    acc = np.zeros((R, R), T)
    for dj in range(-P, P + 1):
        oky = (wy + dj >= 0) & (wy + dj < R)
        for di in range(-P, P + 1):
            w = G[abs(di), abs(dj)] if mistake == "swap" else G[abs(dj), abs(di)]
            en = np.roll(e, (-dj, -di), (0, 1))                                  # [my][mx] = e[my + dj][mx + di]
            if not periodic:
                okx = (wx + di >= 0) & (wx + di < R)
                en = np.where(oky[:, None] & okx[None, :], en, zero)
            acc = acc + w * en
    k = ripple64.sponge_index(wx, wy, R, B)
    v1 = (rate + h * (gs * acc)) * f[k] if mistake == "sign" else (rate - h * (gs * acc)) * f[k]
    e1 = e + h * v1
    assert e1.dtype == T and v1.dtype == T and acc.dtype == T
    return e1, v1


class Layer(ripple64.Layer):
    """ripple64.Layer with datum_ocean_set_ripple_dispersion's mode and g; G the fp32 table the step uses (the library's, where a test has
    it: numpy's cosines may round a weight the other way)"""

    def __init__(self, R, s, dtype=F, c=2.0, gamma=0.05, B=8, sponge_gamma=4.0, mode=DEEP, g=G_DEFAULT, G=None, periodic=False):
        super().__init__(R, s, dtype, c, gamma, B, sponge_gamma)
        self.mode, self.g, self.periodic = mode, g, periodic
        self.G = weights32() if G is None else np.asarray(G, F).reshape(Q, Q)

    def step(self, dt, substeps=1, mistake=None):
        if self.mode == WAVE:
            return super().step(dt, substeps, mistake)
        h, gs, f = params(self.g, self.s, self.gamma, self.B, self.sponge_gamma, dt, substeps, mistake)
        for i in range(substeps):
            self.eta, self.rate = substep(self.eta, self.rate, self.src, self.ox, self.oy, self.B, h, gs, f, self.G, i == 0, self.T, mistake, self.periodic)
            if i == 0:
                self.src = np.zeros_like(self.src)
