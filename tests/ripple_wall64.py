"""Ripple walls (include/datum_ocean_hip.h: "ripple walls") restated, beside ripple_deep64.py and on top of it:

  WALL              the numpy dtype of the 32-byte datum_ocean_ripple_wall; box / ellipse build one record from an angle's cosine and sine;
  raster            the plane [R, R] uint8 in MEMORY order from a list at an origin, in numpy float32 -- every operation one rounding as
                    written, the bits of datum_amd/csrc/ocean_ripple_wall.h -- or in float64;
  substep_wave      one walled WAVE sub-step over the layer in memory order, float32 (the bits) or float64;
  substep_deep      one walled DEEP sub-step;
  Layer             ripple_deep64.Layer with a wall list: center / move rebuild the plane, set_walls zeroes the wall cells' state.

With an all-zero plane both sub-steps are ripple64's and ripple_deep64's bit for bit.

`mistake` plants the errors tests/test_ripple_wall64.py names:
  "wall_zero"       a wall neighbour reads 0 in WAVE                "unpinned"   a wall cell is stepped like water
  "alias_flag"      a neighbour outside the window takes the flag of the torus-aliased cell
  "src_leak"        a wall cell's pending deposit reaches its neighbours' first sub-step (either mode)
  "sine"            the raster with the axis' sine negated
"""

import numpy as np

import ripple64
import ripple_deep64 as rd

F = np.float32
BOX, ELLIPSE = 0, 1
MAX_WALLS = 256
WAVE, DEEP = rd.WAVE, rd.DEEP

MISTAKES = ("wall_zero", "unpinned", "alias_flag", "src_leak", "sine")

WALL = np.dtype([("center", F, 2), ("axis", F, 2), ("half", F, 2), ("kind", np.int32), ("reserved", np.int32)])
assert WALL.itemsize == 32

# The device against float64, for one walled datum_ocean_step_ripples call (up to 16 sub-steps) from a common fp32 state:
# |eta - eta64| <= K eps max|eta64|, one K per mode.  3 x the worst distance of THIS restatement from its float64 form over
# tests/test_ripple_wall_emul.py's cases (measured on the CPU: WAVE 5.88, DEEP 13.48, see that file); the device is the restatement
# bit for bit, so the figures are not taken from the GPU
K_RIP_WALL = {WAVE: 17.7, DEEP: 40.5}


def box(cx, cy, hx, hy, cos=1.0, sin=0.0):
    return np.array([((cx, cy), (cos, sin), (hx, hy), BOX, 0)], WALL)


def ellipse(cx, cy, hx, hy, cos=1.0, sin=0.0):
    return np.array([((cx, cy), (cos, sin), (hx, hy), ELLIPSE, 0)], WALL)


def walls(*records):
    return np.concatenate(records) if records else np.zeros(0, WALL)


def covers(w, x, y, dtype=F, mistake=None):
    """does record w cover the points (x, y)?  arrays of dtype"""
    T = dtype
    cx, cy = T(w["center"][0]), T(w["center"][1])
    ax, ay = T(w["axis"][0]), T(w["axis"][1])
    if mistake == "sine":
        ay = -ay
    h0, h1 = T(w["half"][0]), T(w["half"][1])
    dx, dy = x - cx, y - cy
    u = dx * ax + dy * ay
    v = dy * ax - dx * ay
    if int(w["kind"]) == BOX:
        return (np.abs(u) <= h0) & (np.abs(v) <= h1)
    a, b, r = u * h1, v * h0, h0 * h1
    return a * a + b * b <= r * r


def raster(wl, R, ox, oy, s, dtype=F, mistake=None):
    """[R, R] uint8 in memory order: 1 where any record covers the centre of the world cell the memory cell holds at origin (ox, oy)"""
    T = dtype
    m = np.arange(R)
    I, J = ox + ((m - ox) & (R - 1)), oy + ((m - oy) & (R - 1))
    x = ((I.astype(F).astype(T) + T(0.5)) * T(F(s)))[None, :]
    y = ((J.astype(F).astype(T) + T(0.5)) * T(F(s)))[:, None]
    assert x.dtype == T
    plane = np.zeros((R, R), bool)
    for w in wl:
        plane |= covers(w, x, y, T, mistake)
    return plane.astype(np.uint8)


def _neighbours(a, fill=None):
    """(L, R, D, U): [my][mx] = a[my][mx -/+ 1], a[my -/+ 1][mx] on the torus"""
    return np.roll(a, 1, 1), np.roll(a, -1, 1), np.roll(a, 1, 0), np.roll(a, -1, 0)


def substep_wave(eta, rate, src, wall, ox, oy, B, h, c2s2, f, first, dtype=F, mistake=None):
    """(eta, rate) [R, R] in memory order after one walled WAVE sub-step; wall [R, R] uint8"""
    R = eta.shape[0]
    T = dtype
    eta, rate = eta.astype(T), rate.astype(T)
    h, c2s2, f = T(h), T(c2s2), np.asarray(f).astype(T)
    w = np.asarray(wall) != 0
    e = eta + src.astype(T) * T(ripple64.UNIT) if first else eta
    wx, wy = ripple64.window_coords(R, ox, oy)
    zero = T(0)
    ins = (wx[None, :] != 0, wx[None, :] != R - 1, wy[:, None] != 0, wy[:, None] != R - 1)
    en = []
    dep = e - eta                                         # what the pending deposits add (the planted leak only)
    for n, nw, nd, inside in zip(_neighbours(e), _neighbours(w), _neighbours(dep), ins):
        inside = np.broadcast_to(inside, (R, R))
        if mistake == "alias_flag":
            v = np.where(nw, e, np.where(inside, n, zero))
        elif mistake == "wall_zero":
            v = np.where(inside & ~nw, n, zero)
        elif mistake == "src_leak":
            v = np.where(~inside, zero, np.where(nw, e + nd, n))
        else:
            v = np.where(~inside, zero, np.where(nw, e, n))
        en.append(v)
    eL, eR, eD, eU = en
    k = ripple64.sponge_index(wx, wy, R, B)
    lap = ((eL + eR) + (eD + eU)) - T(4) * e
    v1 = (rate + h * (c2s2 * lap)) * f[k]
    e1 = e + h * v1
    if mistake != "unpinned":
        e1, v1 = np.where(w, zero, e1), np.where(w, zero, v1)
    assert e1.dtype == T and v1.dtype == T
    return e1, v1


def substep_deep(eta, rate, src, wall, ox, oy, B, h, gs, f, G, first, dtype=F, mistake=None):
    """(eta, rate) [R, R] in memory order after one walled DEEP sub-step: ripple_deep64.substep over an image in which wall cells are 0"""
    T = dtype
    w = np.asarray(wall) != 0
    zero = T(0)
    eta, rate = eta.astype(T), rate.astype(T)
    if mistake == "src_leak":
        img, s = np.where(w, zero, eta), src
    else:
        img, s = np.where(w, zero, eta), np.where(w, 0, src).astype(np.int32)
    e1, v1 = rd.substep(img, rate, s, ox, oy, B, h, gs, f, G, first, T)
    if mistake != "unpinned":
        e1, v1 = np.where(w, zero, e1), np.where(w, zero, v1)
    return e1, v1


class Layer(rd.Layer):
    """ripple_deep64.Layer with datum_ocean_set_ripple_walls' list; `wall` is the plane in memory order, None while walls are off"""

    def __init__(self, R, s, dtype=F, c=2.0, gamma=0.05, B=8, sponge_gamma=4.0, mode=WAVE, g=rd.G_DEFAULT, G=None):
        super().__init__(R, s, dtype, c, gamma, B, sponge_gamma, mode=mode, g=g, G=G)
        self.list, self.wall = None, None

    def set_walls(self, wl):
        """the plane, and (+0, +0) in every wall cell (the library zeroes both state buffers; the restatement keeps one)"""
        if wl is None or len(wl) == 0:
            self.list = self.wall = None
            return
        self.list = np.array(wl, WALL)
        self.wall = raster(self.list, self.R, self.ox, self.oy, self.s)
        self.eta[self.wall != 0], self.rate[self.wall != 0] = 0, 0

    def move(self, ox, oy):
        super().move(ox, oy)
        if self.list is not None:
            self.wall = raster(self.list, self.R, self.ox, self.oy, self.s)

    def step(self, dt, substeps=1, mistake=None):
        if self.wall is None:
            return super().step(dt, substeps, mistake)
        if self.mode == WAVE:
            h, c2s2, f = ripple64.params(self.c, self.s, self.gamma, self.B, self.sponge_gamma, dt, substeps)
        else:
            h, gs, f = rd.params(self.g, self.s, self.gamma, self.B, self.sponge_gamma, dt, substeps)
        for i in range(substeps):
            if self.mode == WAVE:
                self.eta, self.rate = substep_wave(self.eta, self.rate, self.src, self.wall, self.ox, self.oy, self.B, h, c2s2, f, i == 0, self.T, mistake)
            else:
                self.eta, self.rate = substep_deep(self.eta, self.rate, self.src, self.wall, self.ox, self.oy, self.B, h, gs, f, self.G, i == 0, self.T, mistake)
            if i == 0:
                self.src = np.zeros_like(self.src)

    def wall_window(self):
        """memory order -> window order, as datum_ocean_read_ripple_walls"""
        return self.window(self.wall)
