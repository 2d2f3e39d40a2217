"""The ripple bed (include/datum_ocean_hip.h: "ripple bed") restated, beside ripple_wall64.py and on top of it:

  BED               the numpy dtype of the 40-byte datum_ocean_ripple_bed; bed() builds one record;
  raster            both planes [R, R] in MEMORY order -- the effective depth (float) and the surf level (uint8) -- from a map, a record, a
                    wall plane or None and an origin, in numpy float32 -- every operation one rounding as written, the bits of
                    datum_amd/csrc/ocean_ripple_bed.h -- or in float64 from the same rounded parameters;
  params            what a step over a bed rounds on the host: h, gs2 = g / s^2, the sponge table and the surf table fsurf[0 .. 16];
  stable            what the call accepts: sqrt(g max_depth) h / s <= 0.7;
  substep           one sub-step over a bed, the layer in memory order, float32 (the bits) or float64;
  Layer             ripple_wall64.Layer with a bed: center / move / set_walls rebuild the planes, set_bed zeroes the solid cells' state.

`mistake` plants the errors tests/test_ripple_bed64.py names:
  "own_depth"       the cell's own depth in place of the face mean        "no_half"      the face coefficient without its 1/2
  "solid_open"      a solid neighbour is not skipped (it reads as water of depth 0 at its height)
  "surf_by_ring"    fsurf indexed by the sponge ring                       "src_own_only" the first sub-step's neighbours lack src
"""

import numpy as np

import ripple64
import ripple_wall64 as rw

F = np.float32
SURF_LEVELS = 16
MAX_SIDE = 4096
WAVE, DEEP = rw.WAVE, rw.DEEP
G_DEFAULT = float(F(9.81))

MISTAKES = ("own_depth", "no_half", "solid_open", "surf_by_ring", "src_own_only")

BED = np.dtype([("width", np.int32), ("height", np.int32), ("origin", F, 2), ("texel", F), ("outside", F), ("max_depth", F), ("dry_depth", F),
                ("surf_depth", F), ("surf_gamma", F)])
assert BED.itemsize == 40

# The device against float64, for one datum_ocean_step_ripples call over a bed (up to 16 sub-steps) from a common fp32 state:
# |eta - eta64| <= K_RIP_BED eps max|eta64|.  3 x the worst distance of THIS restatement from its float64 form over
# tests/test_ripple_bed_emul.py's cases (measured on the CPU: 13.65, see that file's test_k_rip_bed); the device is the restatement bit for
# bit, so the figure is not taken from the GPU
K_RIP_BED = 41.0


def bed(width, height, origin, texel, outside=0.0, max_depth=10.0, dry_depth=0.05, surf_depth=0.0, surf_gamma=0.0):
    return np.array([(width, height, origin, texel, outside, max_depth, dry_depth, surf_depth, surf_gamma)], BED)[0]


def raster(depths, b, wall, R, ox, oy, s, dtype=F):
    """(d [R, R] dtype, q [R, R] uint8) in memory order at origin (ox, oy); depths [height, width] float32, wall [R, R] uint8 or None"""
    T = dtype
    W, H = int(b["width"]), int(b["height"])
    depths = np.asarray(depths, F).reshape(H, W).astype(T)
    invt = T(F(1.0 / float(b["texel"])))
    invsurf = T(F(1.0 / float(b["surf_depth"]))) if b["surf_depth"] > 0 else T(0)
    m = np.arange(R)
    I, J = ox + ((m - ox) & (R - 1)), oy + ((m - oy) & (R - 1))
    x = ((I.astype(F).astype(T) + T(0.5)) * T(F(s)))[None, :]
    y = ((J.astype(F).astype(T) + T(0.5)) * T(F(s)))[:, None]
    u = np.broadcast_to((x - T(b["origin"][0])) * invt, (R, R))
    v = np.broadcast_to((y - T(b["origin"][1])) * invt, (R, R))
    on = (u >= 0) & (u <= T(W - 1)) & (v >= 0) & (v <= T(H - 1))
    us, vs = np.where(on, u, T(0)), np.where(on, v, T(0))
    i = np.minimum(np.floor(us).astype(np.int64), W - 2)
    j = np.minimum(np.floor(vs).astype(np.int64), H - 2)
    wu, wv = us - i.astype(T), vs - j.astype(T)
    c0, c1, c2, c3 = depths[j, i], depths[j, i + 1], depths[j + 1, i], depths[j + 1, i + 1]
    a0, a1 = c1 - c0, c3 - c2
    e0, e1 = c0 + wu * a0, c2 + wu * a1
    raw = np.where(on, e0 + wv * (e1 - e0), T(b["outside"]))
    d = np.minimum(np.maximum(raw, T(0)), T(b["max_depth"]))
    d = np.where(d < T(b["dry_depth"]), T(0), d)
    if wall is not None:
        d = np.where(np.asarray(wall) != 0, T(0), d)
    assert d.dtype == T
    q = np.zeros((R, R), np.uint8)
    if b["surf_depth"] > 0:
        lvl = np.minimum(SURF_LEVELS, np.floor((T(1) - d * invsurf) * T(SURF_LEVELS)).astype(np.int64))
        q = np.where((d == 0) | (d >= T(b["surf_depth"])), 0, lvl).astype(np.uint8)
    return d, q


def params(g, s, gamma, B, sponge_gamma, surf_gamma, dt, substeps):
    """(h, gs2, f, fsurf): h = dt * (1 / substeps) in fp32; gs2, f[0 .. B] and fsurf[0 .. 16] in double from the fp32 parameters, rounded once"""
    h, _, f = ripple64.params(1.0, s, gamma, B, sponge_gamma, dt, substeps)
    g, s, surf_gamma = float(F(g)), float(F(s)), float(F(surf_gamma))
    u = np.arange(SURF_LEVELS + 1, dtype=np.float64) / SURF_LEVELS
    fsurf = (1.0 / (1.0 + float(h) * (surf_gamma * (u * u)))).astype(F)
    return h, F(g / (s * s)), f, fsurf


def stable(g, max_depth, s, dt, substeps):
    h = F(dt) * (F(1) / F(substeps))
    return float(h) >= 0 and np.sqrt(float(F(g)) * float(F(max_depth))) * float(h) / float(F(s)) <= 0.7


def substep(eta, rate, src, d, q, ox, oy, B, h, gs2, f, fsurf, first, dtype=F, mistake=None):
    """(eta, rate) [R, R] in memory order after one sub-step over the bed (d, q)"""
    R = eta.shape[0]
    T = dtype
    eta, rate = eta.astype(T), rate.astype(T)
    h, gs2, f, fsurf = T(h), T(gs2), np.asarray(f).astype(T), np.asarray(fsurf).astype(T)
    d = np.asarray(d).astype(T)
    e = eta + src.astype(T) * T(ripple64.UNIT) if first else eta
    en = eta if (first and mistake == "src_own_only") else e
    wx, wy = ripple64.window_coords(R, ox, oy)
    zero = T(0)
    ins = (wx[None, :] != 0, wx[None, :] != R - 1, wy[:, None] != 0, wy[:, None] != R - 1)
    t = []
    for n, dn, inside in zip(rw._neighbours(en), rw._neighbours(d), ins):
        inside = np.broadcast_to(inside, (R, R))
        if mistake == "own_depth":
            face = d
        elif mistake == "no_half":
            face = d + dn
        else:
            face = T(0.5) * (d + dn)
        wet = face * (n - e)
        if mistake != "solid_open":
            wet = np.where(dn == 0, zero, wet)
        t.append(np.where(inside, wet, d * (zero - e)))
    tL, tR, tD, tU = t
    k = ripple64.sponge_index(wx, wy, R, B)
    fq = fsurf[np.minimum(k, SURF_LEVELS)] if mistake == "surf_by_ring" else fsurf[np.asarray(q, np.int64)]
    fac = f[k] * fq
    div = (tL + tR) + (tD + tU)
    v1 = (rate + h * (gs2 * div)) * fac
    e1 = e + h * v1
    e1, v1 = np.where(d == 0, zero, e1), np.where(d == 0, zero, v1)
    assert e1.dtype == T and v1.dtype == T
    return e1, v1


class Layer(rw.Layer):
    """ripple_wall64.Layer with datum_ocean_set_ripple_bed's map and record; `d` and `q` are the planes in memory order, None while the bed is off"""

    def __init__(self, R, s, dtype=F, c=2.0, gamma=0.05, B=8, sponge_gamma=4.0, mode=WAVE, g=G_DEFAULT, G=None):
        super().__init__(R, s, dtype, c, gamma, B, sponge_gamma, mode=mode, g=g, G=G)
        self.bed, self.depths, self.d, self.q = None, None, None, None

    def _raster(self):
        if self.bed is not None:
            self.d, self.q = raster(self.depths, self.bed, self.wall, self.R, self.ox, self.oy, self.s)

    def set_bed(self, b, depths=None):
        """both planes, and (+0, +0) in every solid cell (the library zeroes both state buffers; the restatement keeps one)"""
        if b is None:
            self.bed = self.depths = self.d = self.q = None
            return
        assert self.mode == WAVE
        self.bed, self.depths = b, np.array(depths, F).reshape(int(b["height"]), int(b["width"]))
        self._raster()
        self.eta[self.d == 0], self.rate[self.d == 0] = 0, 0

    def set_walls(self, wl):
        super().set_walls(wl)
        self._raster()

    def move(self, ox, oy):
        super().move(ox, oy)
        self._raster()

    def step(self, dt, substeps=1, mistake=None):
        if self.bed is None:
            return super().step(dt, substeps, mistake)
        h, gs2, f, fsurf = params(self.g, self.s, self.gamma, self.B, self.sponge_gamma, self.bed["surf_gamma"], dt, substeps)
        for i in range(substeps):
            self.eta, self.rate = substep(self.eta, self.rate, self.src, self.d, self.q, self.ox, self.oy, self.B, h, gs2, f, fsurf, i == 0, self.T, mistake)
            if i == 0:
                self.src = np.zeros_like(self.src)

    def bed_window(self):
        """memory order -> window order, as datum_ocean_read_ripple_bed"""
        return self.window(self.d), self.window(self.q)
