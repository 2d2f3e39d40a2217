"""The physics of coupled stepping (include/datum_ocean_hip.h: "coupled stepping") in float64 on a flat ocean at rest (couple64.Flat64: the
definition's formulas, the layer's sub-step in float64, the deposits the integers they are defined to be).  These tests decide what the
header says about a body that feels its own wake.

Parameters, all tests: water of rho g = 9810 N/m^3 at z = 0; a box of 9 x 9 probes half a metre apart (4 m x 4 m), weight a each, flat
bottom, mass such that its Archimedes draught is D = 0.5 m; the layer's defaults c = 2 m/s, gamma = 0.05 1/s, sponge 8 cells of 4 1/s,
R = 64 cells of s = 0.5 m; sub-steps of h = 0.01 s (c h / s = 0.04; the buoyancy spring's omega h = 0.044).  The ratio a / s^2 is set
through a; the box's mass follows a, so the spring's frequency does not change with it.

WHAT THE SCAN FOUND (test_own_wake_needs_drag).  With no drag the heave of a body that feels its own wake GROWS at every ratio of the
grid 0.01 ... 1: the heave splat lowers the cell under a sinking column, the wave equation fills the hollow, and the filling flow --
water rising relative to the hull -- is read by the next sub-step as the hull sinking further: the source feeds itself.  No ratio is
stable without damping, so none is fixed here or in the header.  The linear drag of the body's motion (cl) is what bounds it: the
excursion never exceeds the drop and decays once cl D >= rho g (a / s^2), in SI numbers, which the test pins at three ratios."""

import numpy as np
import pytest

import body64
import couple64
import drag64
import ripple64
import step64

F = np.float32
RHOG, G, D, H, CELL, R = 9810.0, 9.81, 0.5, 0.01, 0.5, 64
C = 2.0


def _box(a, n=9, half=2.0):
    g = np.linspace(-half, half, n)
    xx, yy = np.meshgrid(g, g)
    p = np.zeros((n * n, 4), F)
    p[:, 0], p[:, 1], p[:, 3] = xx.ravel(), yy.ravel(), a
    return p


def _sim(ratio, cl, centres, drops, couple=True):
    """boxes at `centres` whose bottoms start `drops` metres above the Archimedes draught, at rest"""
    a = ratio * CELL * CELL
    probes = _box(a)
    n, nb = len(probes), len(centres)
    area = n * a
    mass = RHOG * area * D / G
    pos = [[x, y, -D + dz] for (x, y), dz in zip(centres, drops)]
    bodies = body64.make_bodies([np.eye(3)] * nb, pos, [0] * nb, [n] * nb, [np.inf] * nb)
    motions = drag64.make_motions(np.zeros((nb, 3)), np.zeros((nb, 3)), [cl] * nb, [0.0] * nb)
    props = step64.make_props([1.0 / mass] * nb, np.full((nb, 3), 1.0e-4 / ratio), [G] * nb, [RHOG] * nb)
    lay = ripple64.Layer(R, CELL, np.float64)
    return couple64.Flat64(lay, bodies, motions, props, probes, couple), mass, area


def _energy(sim, mass, area):
    """body: kinetic + m g z + the buoyancy's potential of a flat-bottomed box in water at z = 0; layer: the potential of its heights"""
    z, v = sim.T[:, 2], sim.v
    body = 0.5 * mass * (v * v).sum(1) + mass * G * z + 0.5 * RHOG * area * np.maximum(0.0, -z) ** 2
    layer = 0.5 * RHOG * CELL * CELL * float((sim.layer.eta ** 2).sum())
    return float(body.sum()) + layer


def test_dropped_box_settles_to_its_archimedes_draught():
    """ratio 0.25 with cl D = 2500 >= rho g 0.25 = 2452.  The box floats in the water it stands in: its draught is Archimedes' against the
    mean level e of the layer under its probes, which the layer's own damping (gamma = 0.05 1/s) lets die only slowly.  The heave is a
    spring of omega^2 = G / D = 19.6 1/s^2 damped at k = cl G / RHOG = 5 1/s by the drag alone (the layer adds to it): overdamped enough
    that after T = 20 s the transient is below drop exp(-omega^2 T / k) and what is left is the lag of a follower with the time constant
    k / omega^2 behind a level that moves at the layer's rate r under the hull, plus the deposits' quantum of 2^-20 m in 81 cells"""
    cl, drop, steps = 5000.0, 0.3, 2000
    sim, mass, area = _sim(0.25, cl, [(0.1, 0.05)], [drop])
    zs = []
    for _ in range(steps):
        sim.substep(H)
        zs.append(sim.T[0, 2])
    zs = np.array(zs)
    x, y = sim.probes[:, 0] + sim.T[0, 0], sim.probes[:, 1] + sim.T[0, 1]
    eta, rate = sim.sample(x, y)
    k, w2 = cl * G / RHOG, G / D
    bound = drop * np.exp(-w2 * steps * H / k) + k / w2 * np.abs(rate).max() + H * np.abs(rate).max() + 81 * 2.0 ** -20
    assert abs(zs[-1] + D - eta.mean()) <= bound, (zs[-1] + D - eta.mean(), bound)
    assert np.abs(zs + D).max() <= drop and abs(zs[-1] + D) < 0.05 * drop and bound < 0.01 * drop


def test_rings_travel_at_c_and_move_a_second_body_only_after_they_arrive():
    """The rings of a dropped box reach a cell 9.5 cells from its side, and a second box 12 cells from it, at the layer's speed c.  An
    exact zero before the arrival does not exist in float64 -- the stencil carries a trace of 1e-14 one cell per sub-step -- so the front
    is pinned by fractions of the signal's own later peak (the largest value in 6 s), with t_c = distance / c from the first hull's side:
      before 0.5 t_c    the signal is below 1e-3 of its peak     (nothing has arrived: a wave speed of 2 c would have brought it)
      by 1.5 t_c        it has passed 0.1 of its peak, and the peak itself falls in [t_c, 1.5 t_c]   (a speed of c / 2 would not)
    for both signals: |eta| at the cell, and the second box's heave away from a twin that does not feel the layer (the twin carries the
    same residual of the rounded mass, so the difference is the coupling alone)."""
    gap_cells = 12
    x2 = 2.0 + gap_cells * CELL + 2.0
    sim, mass, area = _sim(0.25, 5000.0, [(0.0, 0.0), (x2, 0.0)], [0.3, 0.0])
    off, _, _ = _sim(0.25, 5000.0, [(0.0, 0.0), (x2, 0.0)], [0.3, 0.0], couple=False)
    lay = sim.layer
    I, J = int(np.floor((2.0 + 8 * CELL) / CELL)) + 1, 0                      # a cell more than 8 cells beyond the first hull's side
    idx = ripple64._index(I, J, R)
    steps = 600
    eta, heave = np.zeros(steps), np.zeros(steps)
    for i in range(steps):
        sim.substep(H)
        off.substep(H)
        eta[i], heave[i] = abs(lay.eta.reshape(-1)[idx]), abs(sim.T[1, 2] - off.T[1, 2])
    t = (np.arange(steps) + 1) * H
    for name, sig, dist in (("eta", eta, (I + 0.5) * CELL - 2.0), ("second box", heave, gap_cells * CELL)):
        assert dist >= 8 * CELL
        tc = dist / C
        peak, tpeak = sig.max(), t[sig.argmax()]
        assert peak > 1e-3, (name, peak)
        assert sig[t <= 0.5 * tc].max() < 1e-3 * peak, (name, sig[t <= 0.5 * tc].max() / peak)
        assert sig[t <= 1.5 * tc].max() > 0.1 * peak and tc <= tpeak <= 1.5 * tc, (name, tpeak, tc)
    # without the coupling the second box stays in its equilibrium (but for the residual of the rounded mass)
    assert abs(off.T[1, 2] + D) < 1e-6


GRID = (0.01, 0.05, 0.25, 1.0)
DAMPED = (0.01, 0.05, 0.25)          # at ratio 1 the drag cl D = rho g ratio keeps the excursion below the drop but not the energy below its start


@pytest.mark.parametrize("ratio", GRID)
def test_own_wake_needs_drag(ratio):
    """2000 sub-steps, the sponge on.  Without drag the total of body and layer energy climbs above its start at EVERY ratio of the grid
    (the finding the header states); with cl D >= rho g ratio it never exceeds its start by more than the deposits' rounding, and the
    excursion never exceeds the drop"""
    drop, steps = 0.3, 2000
    free, mass, area = _sim(ratio, 0.0, [(0.1, 0.05)], [drop])
    e0 = _energy(free, mass, area)
    worst, zmax = e0, 0.0
    for _ in range(steps):
        free.substep(H)
        worst, zmax = max(worst, _energy(free, mass, area)), max(zmax, abs(free.T[0, 2] + D))
    scale = 0.5 * RHOG * area * drop * drop                                   # the energy the drop put in
    assert worst > e0 + 0.05 * scale and zmax > 1.05 * drop, (ratio, (worst - e0) / scale, zmax)

    if ratio not in DAMPED:
        return
    cl = RHOG * ratio / D * 1.02
    damped, mass, area = _sim(ratio, cl, [(0.1, 0.05)], [drop])
    e0 = _energy(damped, mass, area)
    worst, zmax = e0, 0.0
    for _ in range(steps):
        damped.substep(H)
        worst, zmax = max(worst, _energy(damped, mass, area)), max(zmax, abs(damped.T[0, 2] + D))
    assert worst <= e0 + 1e-3 * scale and zmax <= drop, (ratio, (worst - e0) / scale, zmax)
    assert abs(damped.T[0, 2] + D) < drop
