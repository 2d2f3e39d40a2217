"""Ripple walls (include/datum_ocean_hip.h: "ripple walls") in float64, through tests/ripple_wall64.py, to 1e-12 (the bar of the closed
forms of the wave step and the DEEP step):

  eigenmodes   a closed basin of m x n open cells walled all round, well inside the window, gamma = 0: cos(pi p (i + 1/2) / m)
               cos(pi q (j + 1/2) / n) stays that mode and follows symplectic Euler's recurrence with
               omega^2 = (c/s)^2 (4 sin^2(pi p / 2m) + 4 sin^2(pi q / 2n)), at three (p, q); the walls stay (+0, +0);
  mirror       a wall column across the whole window at R/2: the walled WAVE run on the left half equals a wall-free run from the
               mirror-symmetrised start restricted to that half, the sponge on; walls and deposits beyond the column change nothing;
  volume       sum eta over the open cells of a closed basin is conserved in WAVE;
  invariant    each mode's invariant v.v + e.Ae - h (Ae).v over the open cells is conserved at gamma = 0 with an irregular wall set;
  deposits     a pending deposit on a wall cell is lost, in both modes;
  no walls     an all-zero plane gives ripple64's and ripple_deep64's results bit for bit;
  raster       a long thin rotated box lies along its axis;
  mistakes     each planted mistake of ripple_wall64.MISTAKES fails at least one assertion above.
"""

import numpy as np
import pytest

import ripple64
import ripple_deep64 as rd
import ripple_wall64 as rw

F = np.float32
R, S, C, H = 64, 0.5, 2.0, 0.1
ZERO = np.zeros((R, R), np.int32)


def _params(mode, gamma=0.0, B=0, sponge_gamma=0.0):
    """(h, coefficient, f) of the mode: c2s2 in WAVE, gs in DEEP"""
    if mode == rw.WAVE:
        return ripple64.params(C, S, gamma, B, sponge_gamma, H, 1)
    return rd.params(rd.G_DEFAULT, S, gamma, B, sponge_gamma, H, 1)


def _sub(mode, eta, rate, src, wall, h, k, f, first=False, B=0, origin=(0, 0), mistake=None):
    if mode == rw.WAVE:
        return rw.substep_wave(eta, rate, src, wall, *origin, B, h, k, f, first, np.float64, mistake)
    return rw.substep_deep(eta, rate, src, wall, *origin, B, h, k, f, rd.weights32(), first, np.float64, mistake)


# -- eigenmodes of a closed basin

M, N, I0, J0 = 20, 13, 17, 23                              # the basin's open cells: columns I0 .. I0 + M - 1, rows J0 .. J0 + N - 1 (memory = window)


def _basin():
    wall = np.zeros((R, R), np.uint8)
    wall[J0 - 1:J0 + N + 1, I0 - 1:I0 + M + 1] = 1
    wall[J0:J0 + N, I0:I0 + M] = 0
    return wall


def _eigen_error(p, q, mistake=None, n=200):
    h, c2s2, f = _params(rw.WAVE)
    h, c2s2 = float(h), float(c2s2)
    w2 = c2s2 * (4 * np.sin(np.pi * p / (2 * M)) ** 2 + 4 * np.sin(np.pi * q / (2 * N)) ** 2)
    cos = 1 - h * h * w2 / 2
    assert abs(cos) < 1
    theta = np.arccos(cos)
    x1 = 1 - h * h * w2
    mode = np.zeros((R, R))
    mode[J0:J0 + N, I0:I0 + M] = np.outer(np.cos(np.pi * q * (np.arange(N) + 0.5) / N), np.cos(np.pi * p * (np.arange(M) + 0.5) / M))
    wall = _basin()
    eta, rate, worst = mode.copy(), np.zeros((R, R)), 0.0
    for k in range(1, n + 1):
        eta, rate = _sub(rw.WAVE, eta, rate, ZERO, wall, h, c2s2, f, mistake=mistake)
        if k in (1, 2, 57, n):
            want = np.cos(k * theta) + (x1 - cos) * np.sin(k * theta) / np.sin(theta)
            worst = max(worst, np.abs(eta - want * mode).max())           # the whole field: walls and the water outside stay 0
    return worst


MODES = [(1, 0), (2, 3), (M - 1, N - 1)]


@pytest.mark.parametrize("p,q", MODES)
def test_eigenmode_closed_form(p, q):
    assert _eigen_error(p, q) < 1e-12


# -- the mirror


def _mirror_error(mistake=None, origin=(37, -21)):
    rng = np.random.default_rng(2)
    B = 8
    h, c2s2, f = ripple64.params(C, S, 0.05, B, 4.0, H, 1)
    shift = (origin[1] & (R - 1), origin[0] & (R - 1))
    mem = lambda a: np.roll(a, shift, (0, 1))                              # window order -> memory order
    win = lambda a: np.roll(a, (-shift[0], -shift[1]), (0, 1))
    half = rng.normal(size=(R, R // 2))
    start = np.concatenate([half, half[:, ::-1]], 1)                         # symmetric about the face between columns R/2 - 1 and R/2
    src = rng.integers(-2 ** 21, 2 ** 21, (R, R // 2)).astype(np.int32)
    src2 = np.concatenate([src, src[:, ::-1]], 1)
    # the walled run: the column at R/2, walls on the window's last column and row beyond it, anything to the right, deposits on all of them
    wall = np.zeros((R, R), np.uint8)
    wall[:, R // 2] = 1
    wall[5:40, R - 1] = 1
    wall[R - 1, R // 2 + 3:] = 1
    wet = np.concatenate([half, rng.normal(size=(R, R // 2))], 1) * (wall == 0)
    wsrc = np.concatenate([src, rng.integers(-2 ** 21, 2 ** 21, (R, R // 2)).astype(np.int32)], 1)
    a, b = (mem(wet), np.zeros((R, R))), (mem(start), np.zeros((R, R)))
    worst = 0.0
    for k in range(40):
        a = rw.substep_wave(*a, mem(wsrc) if k == 0 else ZERO, mem(wall), *origin, B, h, c2s2, f, k == 0, np.float64, mistake)
        b = ripple64.substep(*b, mem(src2) if k == 0 else ZERO, *origin, B, h, c2s2, f, k == 0, np.float64)
        worst = max(worst, np.abs(win(a[0])[:, :R // 2] - win(b[0])[:, :R // 2]).max(), np.abs(win(a[1])[:, :R // 2] - win(b[1])[:, :R // 2]).max())
    assert np.abs(win(b[0])[:, :R // 2]).max() > 0.1
    return worst


def test_mirror():
    assert _mirror_error() < 1e-12


# -- volume


def _volume_drift(mistake=None):
    rng = np.random.default_rng(3)
    h, c2s2, f = _params(rw.WAVE, gamma=0.05)
    wall = _basin()
    eta, rate = rng.normal(size=(R, R)) * (wall == 0), np.zeros((R, R))
    eta[:J0 - 1], eta[J0 + N + 1:], eta[:, :I0 - 1], eta[:, I0 + M + 1:] = 0, 0, 0, 0
    open_ = np.zeros((R, R), bool)
    open_[J0:J0 + N, I0:I0 + M] = True
    v0, drift = eta[open_].sum(), 0.0
    for _ in range(200):
        eta, rate = _sub(rw.WAVE, eta, rate, ZERO, wall, h, c2s2, f, mistake=mistake)
        drift = max(drift, abs(eta[open_].sum() - v0))
    assert abs(v0) > 1
    return drift / np.abs(eta[open_]).sum()


def test_volume_is_conserved():
    assert _volume_drift() < 1e-12


# -- the invariant


def _irregular(origin):
    rng = np.random.default_rng(7)
    x = lambda i: (origin[0] + i + 0.5) * S
    y = lambda j: (origin[1] + j + 0.5) * S
    wl = rw.walls(rw.box(x(20), y(30), 6 * S, 1.3 * S, 0.6, 0.8), rw.ellipse(x(45), y(15), 7 * S, 3 * S, 0.8, -0.6), rw.box(x(0), y(0), 2 * S, 9 * S), rw.box(x(R - 1), y(50), 3 * S, 3 * S))
    wall = rw.raster(wl, R, *origin, S, np.float64)
    wall[rng.random((R, R)) < 0.05] = 1
    return wall


def _invariant_drift(mode, mistake=None, origin=(37, -21)):
    rng = np.random.default_rng(11)
    h, k, f = _params(mode)
    wall = _irregular(origin)
    eta, rate = rng.normal(size=(R, R)) * (wall == 0), rng.normal(size=(R, R)) * (wall == 0)

    def Q(eta, rate):
        # A eta by the restatement itself: one sub-step of length 1 from rest turns eta into the rate -A eta
        Ae = -_sub(mode, eta, np.zeros((R, R)), ZERO, wall, 1.0, k, np.ones(1), origin=origin)[1]
        return float((rate * rate).sum() + (eta * Ae).sum() - float(h) * (Ae * rate).sum())

    q0, drift, pinned = Q(eta, rate), 0.0, 0.0
    for _ in range(100):
        eta, rate = _sub(mode, eta, rate, ZERO, wall, h, k, f, origin=origin, mistake=mistake)
        pinned = max(pinned, np.abs(eta[wall != 0]).max(), np.abs(rate[wall != 0]).max())
        drift = max(drift, abs(Q(eta * (wall == 0), rate * (wall == 0)) - q0) / q0)
    return drift, pinned


@pytest.mark.parametrize("mode", [rw.WAVE, rw.DEEP])
def test_invariant_is_conserved(mode):
    drift, pinned = _invariant_drift(mode)
    assert drift <= 1e-12 and pinned == 0.0


# -- deposits on wall cells


def _deposit_error(mode, mistake=None, origin=(37, -21)):
    rng = np.random.default_rng(13)
    h, k, f = _params(mode, 0.05, 8, 4.0)
    wall = _irregular(origin)
    eta, rate = rng.normal(size=(R, R)) * (wall == 0), rng.normal(size=(R, R)) * (wall == 0)
    water = np.where(wall == 0, rng.integers(-2 ** 21, 2 ** 21, (R, R)), 0).astype(np.int32)
    both = np.where(wall == 0, water, rng.integers(2 ** 20, 2 ** 21, (R, R))).astype(np.int32)
    a = _sub(mode, eta, rate, water, wall, h, k, f, True, 8, origin, mistake)
    b = _sub(mode, eta, rate, both, wall, h, k, f, True, 8, origin, mistake)
    c = _sub(mode, eta, rate, ZERO, wall, h, k, f, True, 8, origin, mistake)
    assert np.abs(a[0] - c[0]).max() > 1e-3                                   # the deposits on water are felt
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())


@pytest.mark.parametrize("mode", [rw.WAVE, rw.DEEP])
def test_wall_deposits_are_lost(mode):
    assert _deposit_error(mode) == 0.0


# -- no walls


@pytest.mark.parametrize("dtype", [F, np.float64])
def test_no_walls_is_the_parent_bit_for_bit(dtype):
    rng = np.random.default_rng(17)
    origin, B = (37, -21), 8
    eta, rate = rng.normal(size=(R, R)).astype(F), rng.normal(size=(R, R)).astype(F)
    src = rng.integers(-2 ** 21, 2 ** 21, (R, R)).astype(np.int32)
    none = np.zeros((R, R), np.uint8)
    G = rd.weights32()
    for first in (True, False):
        h, c2s2, f = ripple64.params(C, S, 0.05, B, 4.0, H, 1)
        got = rw.substep_wave(eta, rate, src, none, *origin, B, h, c2s2, f, first, dtype)
        want = ripple64.substep(eta, rate, src, *origin, B, h, c2s2, f, first, dtype)
        assert all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))
        h, gs, f = rd.params(rd.G_DEFAULT, S, 0.05, B, 4.0, H, 1)
        got = rw.substep_deep(eta, rate, src, none, *origin, B, h, gs, f, G, first, dtype)
        want = rd.substep(eta, rate, src, *origin, B, h, gs, f, G, first, dtype)
        assert all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))
    lay, ref = rw.Layer(R, S, mode=rw.DEEP, G=G), rd.Layer(R, S, G=G)
    for l in (lay, ref):
        l.move(*origin)
        l.set_window(eta, rate, src)
    lay.set_walls(rw.walls())
    lay.step(0.3, 3)
    ref.step(0.3, 3)
    assert lay.wall is None and np.array_equal(lay.state().view(np.uint32), ref.state().view(np.uint32))


# -- the raster's orientation


def _along_axis(mistake=None):
    """a 12 x 1.2 cell box along (0.6, 0.8): the cells five cells out along the axis are wall, those along the mirrored axis are not"""
    wl = rw.box(0.25, 0.25, 6 * S, 0.6 * S, 0.6, 0.8)
    plane = rw.raster(wl, R, -32, -32, S, np.float64, mistake)
    at = lambda I, J: int(plane[J & (R - 1), I & (R - 1)])
    return at(3, 4) + at(-3, -4) + (1 - at(3, -4)) + (1 - at(-3, 4)) + at(0, 0)


def test_box_lies_along_its_axis():
    assert _along_axis() == 5


# -- planted mistakes


def test_planted_mistakes_fail():
    assert set(rw.MISTAKES) == {"wall_zero", "unpinned", "alias_flag", "src_leak", "sine"}
    assert _eigen_error(2, 3, "wall_zero") > 1e-3 and _volume_drift("wall_zero") > 1e-6 and _mirror_error("wall_zero") > 1e-3
    assert _eigen_error(2, 3, "unpinned") > 1e-3
    assert _invariant_drift(rw.WAVE, "unpinned")[1] > 1e-3 and _invariant_drift(rw.DEEP, "unpinned")[1] > 1e-3
    assert _mirror_error("alias_flag") > 1e-3
    assert _deposit_error(rw.WAVE, "src_leak") > 1e-3 and _deposit_error(rw.DEEP, "src_leak") > 1e-3 and _mirror_error("src_leak") > 1e-3
    assert _along_axis("sine") < 5
