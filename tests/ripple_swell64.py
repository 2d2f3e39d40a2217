"""Ripple swell (include/datum_ocean_hip.h: "ripple swell") restated, beside ripple_bed64.py and on top of it:

  solid             which cells are solid, [R, R] bool in MEMORY order: d == 0 over a bed, else the wall byte, else nothing;
  centres           the fp32 centres of the world cells the memory columns and rows hold, as the refresh kernel hands them to the query;
  force             the forcing plane F [R, R] from a plane of heights H (the summed surface above each cell's centre, memory order) and
                    the solid cells, in numpy float32 -- every operation one rounding as written, the bits of
                    datum_amd/csrc/ocean_ripple_swell.h -- or in float64; faces() gives the four differences apart;
  substep_wave      one walled WAVE sub-step with swell, the layer in memory order, float32 (the bits) or float64;
  substep_bed       one WAVE sub-step over a bed with swell;
  Layer             ripple_bed64.Layer with the plane and its CURRENT mark: set_swell / refresh as the library's calls, the mark cleared by
                    move, set_walls, set_bed and set_swell; a step reads F only while the mark stands.

`mistake` plants the errors tests/test_ripple_swell64.py names:
  "flipped"         Hn - Hc for Hc - Hn                                    "solid_forced"  F is not +0 on a solid cell
  "neighbour_depth" over a bed, a face's difference times the neighbour's depth in place of the cell's own
  "after_c2s2"      F added behind the product of c2s2 and the five-point sum
  "stale"           the mark survives a move of the origin
"""

import numpy as np

import ripple64
import ripple_bed64 as rb
import ripple_wall64 as rw

F = np.float32
WAVE, DEEP = rb.WAVE, rb.DEEP

MISTAKES = ("flipped", "neighbour_depth", "solid_forced", "after_c2s2", "stale")

# The device against float64, for one datum_ocean_step_ripples call with swell (up to 16 sub-steps) from a common fp32 state and a common
# fp32 plane F: |eta - eta64| <= K_RIP_SWELL eps max|eta64|.  3 x the worst distance of THIS restatement from its float64 form over
# tests/test_ripple_swell_emul.py's cases (measured on the CPU: 12.97, see that file's test_k_rip_swell); the device is the restatement
# bit for bit, so the figure is not taken from the GPU
K_RIP_SWELL = 39.0

# tests/test_ripple_swell64.py, float64, measured on the CPU by that file and held there: the worst distance of the layer from the mirrored
# wave in front of a straight wall over the amplitude, and rms(H + eta) / rms(H) in the lee of a breakwater, each by cell side in metres
REFLECTION = {1.0: 0.1624, 0.5: 0.0817}
LEE = {1.0: 0.564, 0.5: 0.590}


def solid(wall, d, R):
    if d is not None:
        return np.asarray(d) == 0
    if wall is not None:
        return np.asarray(wall) != 0
    return np.zeros((R, R), bool)


def centres(R, ox, oy, s):
    """(x [R], y [R]) float32: the centre of the world cell that memory column mx (row my) holds at origin (ox, oy)"""
    m = np.arange(R)
    I, J = ox + ((m - ox) & (R - 1)), oy + ((m - oy) & (R - 1))
    return (I.astype(F) + F(0.5)) * F(s), (J.astype(F) + F(0.5)) * F(s)


def points(R, ox, oy, s):
    """[R * R, 2] float32: every cell's centre in memory order, what the heights are asked at"""
    x, y = centres(R, ox, oy, s)
    return np.stack([np.broadcast_to(x[None, :], (R, R)), np.broadcast_to(y[:, None], (R, R))], 2).reshape(-1, 2)


def faces(H, sol, ox, oy, dtype=F, mistake=None):
    """(dL, dR, dD, dU) [R, R]: Hc - Hn where the neighbour counts -- inside the window and solid -- else +0"""
    R = H.shape[0]
    T = dtype
    H = np.asarray(H).astype(T)
    wx, wy = ripple64.window_coords(R, ox, oy)
    ins = (wx[None, :] != 0, wx[None, :] != R - 1, wy[:, None] != 0, wy[:, None] != R - 1)
    out = []
    for Hn, ns, inside in zip(rw._neighbours(H), rw._neighbours(sol), ins):
        counts = np.broadcast_to(inside, (R, R)) & ns
        diff = (Hn - H) if mistake == "flipped" else (H - Hn)
        out.append(np.where(counts, diff, T(0)))
    return out


def force(H, sol, ox, oy, dtype=F, mistake=None):
    """F [R, R] in memory order: (dL + dR) + (dD + dU) on a cell that is not solid, +0 on a solid one"""
    T = dtype
    dL, dR, dD, dU = faces(H, sol, ox, oy, T, mistake)
    Fp = (dL + dR) + (dD + dU)
    if mistake != "solid_forced":
        Fp = np.where(sol, T(0), Fp)
    assert Fp.dtype == T
    return Fp


def substep_wave(eta, rate, src, wall, Fp, ox, oy, B, h, c2s2, f, first, dtype=F, mistake=None):
    """(eta, rate) [R, R] in memory order after one walled WAVE sub-step with swell; wall [R, R] uint8 or None"""
    R = eta.shape[0]
    T = dtype
    eta, rate = eta.astype(T), rate.astype(T)
    h, c2s2, f = T(h), T(c2s2), np.asarray(f).astype(T)
    Fp = np.asarray(Fp).astype(T)
    w = solid(wall, None, R)
    e = eta + src.astype(T) * T(ripple64.UNIT) if first else eta
    wx, wy = ripple64.window_coords(R, ox, oy)
    zero = T(0)
    ins = (wx[None, :] != 0, wx[None, :] != R - 1, wy[:, None] != 0, wy[:, None] != R - 1)
    en = [np.where(~np.broadcast_to(inside, (R, R)), zero, np.where(nw, e, n)) for n, nw, inside in zip(rw._neighbours(e), rw._neighbours(w), ins)]
    eL, eR, eD, eU = en
    k = ripple64.sponge_index(wx, wy, R, B)
    if mistake == "after_c2s2":
        lap = ((eL + eR) + (eD + eU)) - T(4) * e
        v1 = (rate + h * (c2s2 * lap + Fp)) * f[k]
    else:
        lap = (((eL + eR) + (eD + eU)) - T(4) * e) + Fp
        v1 = (rate + h * (c2s2 * lap)) * f[k]
    e1 = e + h * v1
    e1, v1 = np.where(w, zero, e1), np.where(w, zero, v1)
    assert e1.dtype == T and v1.dtype == T
    return e1, v1


def substep_bed(eta, rate, src, d, q, Fp, ox, oy, B, h, gs2, f, fsurf, first, dtype=F, mistake=None, parts=None):
    """(eta, rate) [R, R] in memory order after one WAVE sub-step over the bed (d, q) with swell.  `parts`, the four differences, are
    read by the planted "neighbour_depth" alone"""
    R = eta.shape[0]
    T = dtype
    eta, rate = eta.astype(T), rate.astype(T)
    h, gs2, f, fsurf = T(h), T(gs2), np.asarray(f).astype(T), np.asarray(fsurf).astype(T)
    d, Fp = np.asarray(d).astype(T), np.asarray(Fp).astype(T)
    e = eta + src.astype(T) * T(ripple64.UNIT) if first else eta
    wx, wy = ripple64.window_coords(R, ox, oy)
    zero = T(0)
    ins = (wx[None, :] != 0, wx[None, :] != R - 1, wy[:, None] != 0, wy[:, None] != R - 1)
    t = []
    for n, dn, inside in zip(rw._neighbours(e), rw._neighbours(d), ins):
        wet = np.where(dn == 0, zero, (T(0.5) * (d + dn)) * (n - e))
        t.append(np.where(np.broadcast_to(inside, (R, R)), wet, d * (zero - e)))
    tL, tR, tD, tU = t
    k = ripple64.sponge_index(wx, wy, R, B)
    fac = f[k] * fsurf[np.asarray(q, np.int64)]
    if mistake == "neighbour_depth":
        sL, sR, sD, sU = (dn * np.asarray(p).astype(T) for dn, p in zip(rw._neighbours(d), parts))
        div = ((tL + tR) + (tD + tU)) + ((sL + sR) + (sD + sU))
    else:
        div = ((tL + tR) + (tD + tU)) + d * Fp
    v1 = (rate + h * (gs2 * div)) * fac
    e1 = e + h * v1
    e1, v1 = np.where(d == 0, zero, e1), np.where(d == 0, zero, v1)
    assert e1.dtype == T and v1.dtype == T
    return e1, v1


class Layer(rb.Layer):
    """ripple_bed64.Layer with datum_ocean_set_ripple_swell's plane: `F` in memory order, None while swell is off; `current` the mark"""

    def __init__(self, R, s, dtype=F, c=2.0, gamma=0.05, B=8, sponge_gamma=4.0, mode=WAVE, g=rb.G_DEFAULT, G=None):
        super().__init__(R, s, dtype, c, gamma, B, sponge_gamma, mode=mode, g=g, G=G)
        self.F, self.parts, self.current = None, None, False

    def set_swell(self, on):
        assert not (on and self.mode != WAVE)
        self.F = np.zeros((self.R, self.R), self.T) if on else None
        self.parts, self.current = None, False

    def solid(self):
        return solid(self.wall, self.d, self.R)

    def points(self):
        return points(self.R, self.ox, self.oy, self.s)

    def refresh(self, H, mistake=None):
        """datum_ocean_refresh_ripple_swell with the heights handed in: H [R, R] in memory order, or a function of (x [1, R], y [R, 1])"""
        assert self.F is not None
        if callable(H):
            x, y = centres(self.R, self.ox, self.oy, self.s)
            H = np.broadcast_to(H(x.astype(self.T)[None, :], y.astype(self.T)[:, None]), (self.R, self.R))
        self.parts = faces(H, self.solid(), self.ox, self.oy, self.T, mistake)
        self.F = force(H, self.solid(), self.ox, self.oy, self.T, mistake)
        self.current = True

    def set_walls(self, wl):
        super().set_walls(wl)
        self.current = False

    def set_bed(self, b, depths=None):
        super().set_bed(b, depths)
        self.current = False

    def move(self, ox, oy, mistake=None):
        moved = (ox, oy) != (self.ox, self.oy)
        super().move(ox, oy)
        if moved and mistake != "stale":
            self.current = False

    def step(self, dt, substeps=1, mistake=None):
        # (swell without walls and without a bed: nothing is solid, F is +0 everywhere, and the library launches the plain parent)
        if self.F is None or not self.current or (self.wall is None and self.bed is None):
            return super().step(dt, substeps, None if mistake in MISTAKES else mistake)
        if self.bed is not None:
            h, gs2, f, fsurf = rb.params(self.g, self.s, self.gamma, self.B, self.sponge_gamma, self.bed["surf_gamma"], dt, substeps)
        else:
            h, c2s2, f = ripple64.params(self.c, self.s, self.gamma, self.B, self.sponge_gamma, dt, substeps)
        for i in range(substeps):
            if self.bed is not None:
                self.eta, self.rate = substep_bed(self.eta, self.rate, self.src, self.d, self.q, self.F, self.ox, self.oy, self.B, h, gs2, f, fsurf, i == 0, self.T, mistake, self.parts)
            else:
                self.eta, self.rate = substep_wave(self.eta, self.rate, self.src, self.wall, self.F, self.ox, self.oy, self.B, h, c2s2, f, i == 0, self.T, mistake)
            if i == 0:
                self.src = np.zeros_like(self.src)
