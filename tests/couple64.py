"""Coupled stepping (include/datum_ocean_hip.h: datum_ocean_step_bodies_coupled) restated from body64, drag64, step64 and ripple64 alone,
which all take the probes' records as an argument:

  ripple32      the rippled records: field 2 gets the layer's height added, field 6 its rate, one fp32 addition each;
  substep32     one coupled sub-step in numpy float32, the bits of the device: body64.reduce32, drag64.reduce32 and ripple64.wake32 on the
                rippled records, step64.integrate32, then layer.step(h, 1);
  fold32        a call's record from sub-step to sub-step: fields 7 and 11 by fmaxf and one addition;
  call32        `substeps` coupled sub-steps from per-sub-step velocity records;
  Flat64        the same loop in float64 over a flat, resting ocean (the velocity record is rec[2] = 0, rec[4:7] = 0 everywhere), for the
                physics of tests/test_couple64.py.

`mistake` plants the errors tests/test_couple_emul.py names:
  "no_rate"         the height is added but not the rate          "sample_late"     the sample sees the deposits that are pending
  "wake_unrippled"  the wake is formed from the plain record      "dropped_last"    field 11 is overwritten, not summed
"""

import numpy as np

import body64
import drag64
import ripple64
import step64

F = np.float32

RECORD_FLOATS = 12
MISTAKES = ("no_rate", "sample_late", "wake_unrippled", "dropped_last")


def ripple32(recs, samples, mistake=None):
    """[rows, 8] float32 rippled records from velocity records [rows, 8] and ripple samples [rows, 4] (height, d/dx, d/dy, rate)"""
    recs = np.asarray(recs, F).reshape(-1, 8)
    samples = np.asarray(samples, F).reshape(-1, 4)
    out = recs.copy()
    with np.errstate(all="ignore"):
        out[:, 2] = recs[:, 2] + samples[:, 0]
        if mistake != "no_rate":
            out[:, 6] = recs[:, 6] + samples[:, 3]
    assert out.dtype == F
    return out


def points32(bodies, probes):
    """[rows, 2] float32: (w.x, w.y) of every probe of every body, where its records are taken"""
    w, _, _ = body64.world32(bodies, np.asarray(probes, F).reshape(-1, 4))
    return np.ascontiguousarray(w[:, :2])


def fold32(rec, old, first, mistake=None):
    """the record of a sub-step folded with the record the sub-step before left: rows of NaNs stay NaNs"""
    out = rec.copy()
    if not first:
        with np.errstate(all="ignore"):
            out[:, 7] = np.fmax(old[:, 7], rec[:, 7])
            if mistake != "dropped_last":
                out[:, 11] = old[:, 11] + rec[:, 11]
        out[np.isnan(old[:, 0]) | np.isnan(rec[:, 0])] = np.nan
    return out


def substep32(layer, bodies, motions, props, probes, recs, h, samples=None, old=None, mistake=None, trace=None):
    """One coupled sub-step of length h (a float32).  recs [rows, 8]: the velocity records at points32(bodies, probes); samples: the layer's
    samples there (taken from `layer` when None).  old: the records the sub-step before left, None in a call's first sub-step.  `layer` (a
    float32 ripple64.Layer) is advanced in place; `trace`, a list, receives the sub-step's own record before the fold.  Returns (bodies',
    motions', records [n, 12], bad [n])"""
    probes = np.asarray(probes, F).reshape(-1, 4)
    h = F(h)
    first = old is None
    if samples is None:
        samples = layer.sample(points32(bodies, probes))
    if mistake == "sample_late":
        seen = np.stack([layer.eta + layer.src.astype(F) * ripple64.UNIT, layer.rate], 2)
        samples = ripple64.sample32(seen, layer.ox, layer.oy, layer.invs, points32(bodies, probes))
    rr = ripple32(recs, samples, mistake)
    wasbad = np.zeros(len(bodies), bool) if first else np.isnan(old[:, 0])
    # a body that is bad before the walk -- its props, or an earlier sub-step -- walks no probe: for the wake that is a bad motion
    dead = wasbad | step64.props_bad(props)
    mo = motions.copy()
    mo["linear"][dead] = np.nan
    lift = body64.reduce32(bodies, probes, rr)
    drag = drag64.reduce32(bodies, motions, probes, rr)
    wake = ripple64.wake32(bodies, mo, probes, recs if mistake == "wake_unrippled" else rr, h, layer.src, layer.ox, layer.oy, layer.invs)
    nb, nm, rec8, bad = step64.integrate32(lift, drag, bodies, motions, props, h)
    bad = bad | dead
    rec = np.concatenate([rec8, wake[:, :4]], 1)
    nb[bad], nm[bad], rec[bad] = bodies[bad], motions[bad], np.nan
    if trace is not None:
        trace.append(rec.copy())
    rec = fold32(rec, old, first, mistake)
    assert rec.dtype == F and rec.shape[1] == RECORD_FLOATS
    layer.step(h, 1)
    return nb, nm, rec, bad


def call32(layer, bodies, motions, props, probes, recs_of, dt, substeps, mistake=None, trace=None):
    """datum_ocean_step_bodies_coupled: recs_of(bodies) gives the velocity records [rows, 8] for the poses of a sub-step"""
    h = step64.step_size(dt, substeps)
    rec = None
    for _ in range(substeps):
        bodies, motions, rec, _ = substep32(layer, bodies, motions, props, probes, recs_of(bodies), h, old=rec, mistake=mistake, trace=trace)
    return bodies, motions, rec


def flat_recs(rows):
    """the velocity records of a flat ocean at rest: height 0, residual 0, no velocity"""
    return np.zeros((rows, 8), F)


class Flat64:
    """Bodies on a flat ocean at rest with the ripple layer, in float64: the definition's formulas -- buoyancy and drag per probe from the
    rippled record, the wake's splats (integers, as they are defined), step64.integrate64, the layer's sub-step in float64.  A probe's
    weight a and the cell side s set a / s^2.  couple=False: the bodies do not feel the layer (they still deposit)"""

    def __init__(self, layer, bodies, motions, props, probes, couple=True):
        assert layer.T is np.float64
        self.layer, self.props, self.couple = layer, props, couple
        self.probes = np.asarray(probes, np.float64).reshape(-1, 4)
        self.bi, self.pi = body64._gather(bodies, self.probes)
        self.first, self.count, self.cap = bodies["first"].copy(), bodies["count"].copy(), bodies["cap"].astype(np.float64)
        self.R = bodies["rotation"].astype(np.float64).reshape(-1, 3, 3)
        self.T = bodies["position"].astype(np.float64)
        self.v = motions["linear"].astype(np.float64)
        self.o = motions["angular"].astype(np.float64)
        self.cl, self.cq = motions["cl"].astype(np.float64), motions["cq"].astype(np.float64)
        self.dropped = 0

    def sample(self, x, y):
        """(height, rate) in float64: ripple_sample's bilinear patch, cells outside the window 0"""
        L = self.layer
        invs = float(L.invs)
        out = []
        ux, uy = x * invs - 0.5, y * invs - 0.5
        I0, J0 = np.floor(ux).astype(np.int64), np.floor(uy).astype(np.int64)
        wx, wy = ux - I0, uy - J0
        for plane in (L.eta, L.rate):
            flat = plane.reshape(-1)
            c = []
            for k in range(4):
                I, J = I0 + (k & 1), J0 + (k >> 1)
                c.append(np.where(ripple64._inside(I, J, L.R, L.ox, L.oy), flat[ripple64._index(I, J, L.R)], 0.0))
            e0, e1 = c[0] + wx * (c[1] - c[0]), c[2] + wx * (c[3] - c[2])
            out.append(e0 + wy * (e1 - e0))
        return out

    def substep(self, h):
        L, bi = self.layer, self.bi
        h = float(h)
        p = self.probes[self.pi]
        w = np.einsum("nij,nj->ni", self.R[bi], p[:, :3]) + self.T[bi]
        a = p[:, 3]
        eta, rate = self.sample(w[:, 0], w[:, 1]) if self.couple else (np.zeros(len(w)), np.zeros(len(w)))
        cap = self.cap[bi]
        d = np.minimum(np.maximum(eta - w[:, 2], 0.0), cap)
        m = a * d
        r = w - self.T[bi]
        vel = np.stack([np.zeros(len(w)), np.zeros(len(w)), rate], 1)
        f, tau, e, _ = drag64.terms64(r, self.v[bi], self.o[bi], self.cl[bi], self.cq[bi], m, vel)
        n = len(self.T)
        lift, drag = np.zeros((n, 8)), np.zeros((n, 8))
        np.add.at(lift[:, 0], bi, m)
        np.add.at(lift[:, 1], bi, r[:, 1] * m)
        np.add.at(lift[:, 2], bi, -(r[:, 0] * m))
        for k in range(3):
            np.add.at(drag[:, k], bi, f[:, k])
            np.add.at(drag[:, 3 + k], bi, tau[:, k])
        # the wake of the pose and motion at the start of the sub-step
        heave, wet = (0.0 < d) & (d < cap), d > 0.0
        sx, sy = -(e[:, 0] * h), -(e[:, 1] * h)
        for x, y, V, mask in ((w[:, 0], w[:, 1], (a * -e[:, 2]) * h, heave), (w[:, 0], w[:, 1], -m, wet), (w[:, 0] + sx, w[:, 1] + sy, m, wet)):
            self.dropped += int(ripple64.splat32(L.src, L.ox, L.oy, L.invs, x[mask], y[mask], V[mask]).sum())
        # (integrate64 takes the state from arrays with these fields: hand it the float64 state itself)
        b64 = np.zeros(n, np.dtype([("rotation", np.float64, 9), ("position", np.float64, 3)]))
        b64["rotation"], b64["position"] = self.R.reshape(-1, 9), self.T
        m64 = np.zeros(n, np.dtype([("linear", np.float64, 3), ("angular", np.float64, 3)]))
        m64["linear"], m64["angular"] = self.v, self.o
        out = step64.integrate64(lift, drag, b64, m64, self.props, np.float64(h))
        self.R, self.T, self.v, self.o = out["rotation"].reshape(-1, 3, 3), out["position"], out["linear"], out["angular"]
        self.force = out["force"]
        L.step(h, 1)
        return out
