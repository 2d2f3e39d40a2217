"""Ripple swell's model (include/datum_ocean_hip.h: "ripple swell") in float64, on the CPU, through tests/ripple_swell64.py:

  * the algebra of F: the walled operator applied to the layer plus F equals the walled operator applied to H + eta less the open-sea
    operator applied to H, on every wet cell, to rounding.  That is the definition of F said twice: it guards a sign or a mask, no more;
  * F is +0 on every solid cell and on every cell with no counting neighbour; a neighbour outside the window never counts;
  * over a bed a solid neighbour's term is dc (Hc - Hn), and a beach's source falls with dc;
  * the five planted mistakes each fail one of the above.

The reflection and the lee, the two tests that show the feature doing what it is for, time-step the float64 restatement with gamma = 0,
one sub-step a call and a refresh before each, under an incident plane wave whose omega is the discrete scheme's own for its k:

  * a straight wall across a channel: behind the front that leaves the wall at t = 0 the layer is the mirrored wave.  The incident
    wave's phase is chosen so that H is 0 on the wall's face at t = 0: a wall that appears in a running wave leaves, by d'Alembert,
    H(face, 0) behind the front as a constant that in one dimension never decays (measured: 0.99, 0.08 and 0.73 of the amplitude at
    s = 1, 0.5, 0.25 m with the phase left to chance -- the cosine of k x_face each time), and that offset is the sudden start's, not the
    reflection's.  The error falls with the cell size, first order; the finer run is held to three times its measured error; the total
    field at the cells before the wall evolves by its wet faces alone -- no flux of H + eta through the wall's faces -- to rounding;
  * behind a breakwater three metres thick and four wavelengths wide H + eta is smaller than H alone.
"""

import os

import numpy as np
import pytest

import ripple64
import ripple_bed64 as rb
import ripple_swell64 as rs
import ripple_wall64 as rw
from test_ripple_bed_emul import shore
from test_ripple_swell_emul import ORIGINS, harbour, heights

S = 0.5
D = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _walled_lap(e, sol, ox, oy):
    """the walled five-point sum of a field on the wet cells: a solid neighbour inside the window reads the cell's own value, one outside
    the window 0"""
    R = e.shape[0]
    wx, wy = ripple64.window_coords(R, ox, oy)
    ins = (wx[None, :] != 0, wx[None, :] != R - 1, wy[:, None] != 0, wy[:, None] != R - 1)
    n = [np.where(~np.broadcast_to(i, (R, R)), 0.0, np.where(ns, e, v)) for v, ns, i in zip(rw._neighbours(e), rw._neighbours(sol), ins)]
    return ((n[0] + n[1]) + (n[2] + n[3])) - 4.0 * e


def _open_lap(e, ox, oy, edge):
    """the open-sea five-point sum; `edge` is what a neighbour outside the window reads (the incident field goes on there: its own values)"""
    R = e.shape[0]
    wx, wy = ripple64.window_coords(R, ox, oy)
    ins = (wx[None, :] != 0, wx[None, :] != R - 1, wy[:, None] != 0, wy[:, None] != R - 1)
    n = [np.where(np.broadcast_to(i, (R, R)), v, g) for v, g, i in zip(rw._neighbours(e), edge, ins)]
    return ((n[0] + n[1]) + (n[2] + n[3])) - 4.0 * e


def _identity_residual(mistake=None, R=64, origin=ORIGINS[0]):
    """max over the wet cells off the window's edge of | walled(eta) + F - (walled(H + eta) - open(H)) |, relative to max |H|"""
    rng = np.random.default_rng(3)
    lay = rs.Layer(R, S, D)
    lay.move(*origin)
    lay.set_walls(harbour(R, *origin))
    lay.set_swell(True)
    H = heights(R, *origin, seed=5).astype(D)
    eta = np.where(lay.solid(), 0.0, rng.normal(size=(R, R)))
    lay.refresh(H, mistake)
    sol = lay.solid()
    wx, wy = ripple64.window_coords(R, *origin)
    inner = (wx[None, :] > 0) & (wx[None, :] < R - 1) & (wy[:, None] > 0) & (wy[:, None] < R - 1) & ~sol
    lhs = _walled_lap(eta, sol, *origin) + lay.F
    rhs = _walled_lap(H + eta, sol, *origin) - _open_lap(H, *origin, rw._neighbours(H))
    return float(np.abs(lhs - rhs)[inner].max() / np.abs(H).max()), lay


def test_scattered_field_identity():
    """the algebra of F and of the walled operator agree: a guard against a slip of sign or mask, not a measurement (the flux check is
    test_reflection_off_a_straight_wall's)"""
    res, lay = _identity_residual()
    assert res < 1e-13 and (lay.F != 0).sum() > 60


# -- the reflection and the lee: the incident wave, time-stepped

A, LAM, C, COURANT = 0.5, 8.0, 2.0, 0.4


def _wave(s):
    """(k, omega, h): the scheme's own omega for k along x, sin(omega h / 2) = (c h / s) sin(k s / 2); h is the fp32 the call takes"""
    k, h = 2 * np.pi / LAM, float(np.float32(COURANT * s / C))
    return k, 2 / h * np.arcsin((C * h / s) * np.sin(k * s / 2)), h


def _reflection(R, s, T=24.0, thick=4):
    """a channel along x, 64 m long: walls on the window's first and last rows, a wall `thick` cells deep across its end.  Returns the
    worst distance of the layer from the mirrored wave within two wavelengths of the wall, over the amplitude, and the worst flux residual"""
    L = R * s
    lay = rs.Layer(R, s, D, c=C, gamma=0.0, B=0, sponge_gamma=0.0)
    lay.move(0, 0)
    lay.set_walls(rw.walls(rw.box(L - thick * s / 2, L / 2, thick * s / 2, L), rw.box(L / 2, 0.5 * s, L, 0.3 * s), rw.box(L / 2, L - 0.5 * s, L, 0.3 * s)))
    lay.set_swell(True)
    k, om, h = _wave(s)
    face = (R - thick) * s
    x = rs.centres(R, 0, 0, s)[0].astype(D)
    H = lambda t: np.broadcast_to(A * np.sin(k * (x - face) - om * t)[None, :], (R, R))
    n = int(round(T / h))
    # the reflected front has passed the two wavelengths before the wall, and what the window's far edge sends back has not reached them
    assert 2 * LAM < C * T < 2 * face - 2 * LAM
    prev = None
    for i in range(n + 1):
        prev, now = now if i else None, H(i * h) + lay.eta
        lay.refresh(H(i * h))
        lay.step(h, 1)
    nxt = H((n + 1) * h) + lay.eta
    # the total field at the last wet column, rows off the channel's walls: its second difference in time is (c h / s)^2 times the sum
    # over its WET faces alone -- left, down, up -- so nothing passed the wall's face
    j, i = slice(2, R - 2), R - thick - 1
    wet = (now[j, i - 1] - now[j, i]) + (now[2 - 1:R - 2 - 1, i] - now[j, i]) + (now[2 + 1:R - 2 + 1, i] - now[j, i])
    flux = np.abs((nxt[j, i] - 2 * now[j, i] + prev[j, i]) - (C * h / s) ** 2 * wet).max() / A
    # (one more step was taken: the layer is at t = (n + 1) h)
    mirror = A * np.sin(k * (face - x) - om * (n + 1) * h)
    sel = (x > face - 2 * LAM) & (x < face)
    return float(np.abs(lay.eta[R // 2][sel] - mirror[sel]).max() / A), float(flux)


def test_reflection_off_a_straight_wall():
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    coarse, fc = _reflection(64, 1.0)
    fine, ff = _reflection(128, 0.5)
    print(f"reflection off a straight wall: |eta - mirror| / A = {coarse:.4f} at s = 1 m, {fine:.4f} at s = 0.5 m; flux residual {fc:.1e}, {ff:.1e}")
    assert fc < 1e-12 and ff < 1e-12
    assert fine < 0.6 * coarse                                              # it falls with the cell size (first order: about a half)
    assert fine <= 3 * rs.REFLECTION[0.5] and coarse <= 3 * rs.REFLECTION[1.0]
    assert 0.9 * rs.REFLECTION[0.5] <= fine and 0.9 * rs.REFLECTION[1.0] <= coarse   # the recorded figures are these runs'
    assert f"{rs.REFLECTION[1.0]:.4f} at `s` = 1 m" in design and f"{rs.REFLECTION[0.5]:.4f} at `s` = 0.5 m" in design


def _lee(R, s, T=32.0):
    """rms(H + eta) / rms(H) over the last period, in the 8 m x 12 m of water from 1 m behind a breakwater 3 m thick and 32 m wide that
    stands across the middle of a 64 m window whose sponge takes the scattered field at the edges"""
    L = R * s
    lay = rs.Layer(R, s, D, c=C, gamma=0.0, B=8, sponge_gamma=4.0)
    lay.move(0, 0)
    lay.set_walls(rw.box(31.5, L / 2, 1.5, 16.0))
    lay.set_swell(True)
    k, om, h = _wave(s)
    x, y = (v.astype(D) for v in rs.centres(R, 0, 0, s))
    X, Y = np.broadcast_to(x[None, :], (R, R)), np.broadcast_to(y[:, None], (R, R))
    reg = (X > 34) & (X < 42) & (Y > 26) & (Y < 38)
    H = lambda t: A * np.sin(k * (X - 30.0) - om * t)
    n, per = int(round(T / h)), int(round(2 * np.pi / om / h))
    total = alone = 0.0
    for i in range(n):
        lay.refresh(H(i * h))
        lay.step(h, 1)
        if i >= n - per:
            Hn = H((i + 1) * h)
            total, alone = total + ((Hn + lay.eta)[reg] ** 2).sum(), alone + (Hn[reg] ** 2).sum()
    return float(np.sqrt(total / alone))


def test_lee_of_a_breakwater():
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    coarse, fine = _lee(64, 1.0), _lee(128, 0.5)
    print(f"lee of a breakwater: rms(H + eta) / rms(H) = {coarse:.3f} at s = 1 m, {fine:.3f} at s = 0.5 m")
    assert coarse < 1 and fine < 1
    # the finer run keeps at least a third of the deficit it was measured to have
    assert 1 - fine >= (1 - rs.LEE[0.5]) / 3 and abs(fine - rs.LEE[0.5]) < 0.01 and abs(coarse - rs.LEE[1.0]) < 0.01
    assert f"{rs.LEE[1.0]:.3f} at `s` = 1 m" in design and f"{rs.LEE[0.5]:.3f} at `s` = 0.5 m" in design


def test_zero_where_nothing_counts_and_outside_never_counts():
    for bed in (False, True):
        for origin in ORIGINS:
            R = 64
            lay = rs.Layer(R, S, D)
            lay.move(*origin)
            lay.set_walls(harbour(R, *origin))
            if bed:
                lay.set_bed(*shore(R, *origin))
            lay.set_swell(True)
            lay.refresh(heights(R, *origin, seed=2).astype(D))
            sol = lay.solid()
            nb = sum(n.astype(int) for n in rw._neighbours(sol))
            assert not lay.F[sol].any() and not lay.F[~sol & (nb == 0)].any() and not np.signbit(lay.F[sol]).any()
    # a wall on the window's last column: the first column's cells are its torus neighbours in memory, and do not count it
    R, origin = 64, ORIGINS[0]
    lay = rs.Layer(R, S, D)
    lay.move(*origin)
    lay.set_walls(rw.box((origin[0] + R - 0.5) * S, (origin[1] + R / 2) * S, 0.3 * S, 40 * S))
    lay.set_swell(True)
    lay.refresh(heights(R, *origin, seed=2).astype(D))
    Fw = lay.window(lay.F)
    assert lay.window(lay.wall)[:, R - 1].all() and not Fw[:, 0].any() and (Fw[:, R - 2] != 0).all()


def test_bed_term_is_the_cells_own_depth_and_fades_on_a_beach():
    """one sub-step from rest over a bed: the rate of a wet cell beside solid ones is h gs2 dc F f, F the sum of its (Hc - Hn).  Two
    shelves of different depth that end in the same shoreline under the same H have the same F there, and the rates are as the depths:
    a beach's source falls with dc"""
    R, origin = 64, (0, 0)
    W = 80
    X = -2.0 + 0.5 * np.arange(W)
    x, y = rs.centres(R, *origin, S)
    H = np.broadcast_to(0.3 * np.sin(0.7 * x.astype(D))[None, :] + 0.1 * np.cos(0.5 * y.astype(D))[:, None], (R, R))
    out = {}
    for shelf in (0.8, 0.1):
        depths = np.broadcast_to(np.where(X < 20.0, shelf, -1.0), (W, W)).astype(np.float32)          # water of one depth, land beyond x = 20
        b = rb.bed(W, W, (-2.0, -2.0), 0.5, outside=shelf, max_depth=1.2, dry_depth=0.02)
        lay = rs.Layer(R, S, D, gamma=0.0, B=0)
        lay.move(*origin)
        lay.set_bed(b, depths)
        lay.set_swell(True)
        lay.refresh(H)
        shoreline = ~lay.solid() & np.roll(lay.solid(), -1, 1)              # wet cells whose right neighbour is land
        assert shoreline.sum() == R and (lay.F[shoreline] != 0).all()
        h, gs2, f, fsurf = rb.params(lay.g, lay.s, 0.0, 0, 0.0, 0.0, 0.1, 1)
        lay.step(0.1, 1)
        want = float(h) * (float(gs2) * (lay.d * lay.F))
        assert np.allclose(lay.rate[shoreline], want[shoreline], rtol=1e-12, atol=0) and np.abs(lay.rate[shoreline]).min() > 0
        out[shelf] = shoreline, lay.F[shoreline], lay.rate[shoreline], lay.d[shoreline]
    deep, shallow = out[0.8], out[0.1]
    assert np.array_equal(deep[0], shallow[0]) and np.array_equal(deep[1], shallow[1])                # the same cells, the same F
    assert np.allclose(deep[3] / shallow[3], 8.0, rtol=1e-6) and np.allclose(deep[2] / shallow[2], deep[3] / shallow[3], rtol=1e-12)


@pytest.mark.parametrize("mistake", rs.MISTAKES)
def test_planted_mistakes_fail(mistake):
    R, origin = 64, ORIGINS[0]
    if mistake == "flipped":
        res, _ = _identity_residual(mistake)
        assert res > 1e-2
    elif mistake == "solid_forced":
        _, lay = _identity_residual(mistake)
        assert lay.F[lay.solid()].any()
    elif mistake in ("after_c2s2", "neighbour_depth"):
        bed = mistake == "neighbour_depth"
        out = []
        for m in (None, mistake):
            lay = rs.Layer(R, S, D, gamma=0.0, B=0)
            lay.move(*origin)
            lay.set_walls(harbour(R, *origin))
            if bed:
                lay.set_bed(*shore(R, *origin))
            lay.set_swell(True)
            lay.refresh(heights(R, *origin, seed=5).astype(D))
            lay.step(0.1, 1, mistake=m)
            out.append(lay.rate.copy())
        boundary = lay.F != 0
        assert np.abs(out[0][boundary]).min() > 0 and np.abs(out[1] - out[0])[boundary].max() > 1e-3 * np.abs(out[0]).max()
        if bed:
            assert not out[1][boundary].any()                              # a solid neighbour's depth is 0: the source is gone
    else:
        assert mistake == "stale"
        lay, par = (rs.Layer(R, S, D) for _ in range(2))
        for l in (lay, par):
            l.move(*origin)
            l.set_walls(harbour(R, *origin))
        lay.set_swell(True)
        lay.refresh(heights(R, *origin, seed=5).astype(D))
        lay.move(origin[0] + 3, origin[1] - 2, mistake="stale")
        par.move(origin[0] + 3, origin[1] - 2)
        lay.step(0.1, 1)
        par.step(0.1, 1)
        assert lay.current and not np.array_equal(lay.state(), par.state())
        # as it should be: the mark is cleared, the step is the parent's
        good = rs.Layer(R, S, D)
        good.move(*origin)
        good.set_walls(harbour(R, *origin))
        good.set_swell(True)
        good.refresh(heights(R, *origin, seed=5).astype(D))
        good.move(origin[0] + 3, origin[1] - 2)
        good.step(0.1, 1)
        assert not good.current and np.array_equal(good.state(), par.state())
