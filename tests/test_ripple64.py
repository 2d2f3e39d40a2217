"""The ripple layer's scheme (tests/ripple64.py, the restatement of include/datum_ocean_hip.h) against what is known in closed form.

With B = 0 and gamma = 0 the mode sin(pi p (i+1)/(R+1)) sin(pi q (j+1)/(R+1)) is an eigenvector of the five-point Laplacian with a zero
border, eigenvalue -|lambda|, |lambda| = (4/s^2)(sin^2(pi p/(2(R+1))) + sin^2(pi q/(2(R+1)))).  One sub-step maps its amplitude pair
(a, b) = (height, rate) to b' = b - h w^2 a, a' = a + h b' with w^2 = c^2 |lambda|: a rotation by theta, cos theta = 1 - h^2 w^2 / 2.
With x_n the height amplitude, x_{n+1} = 2 cos(theta) x_n - x_{n-1}, so x_n = x_0 cos(n theta) + (x_1 - x_0 cos theta) sin(n theta) / sin theta.

Energy.  The step is symplectic Euler; per mode its invariant is b^2 + w^2 a^2 - h w^2 a b, in space
    E = 1/2 sum v^2 + 1/2 c2s2 sum |grad e|^2 + 1/2 h c2s2 sum v lap(e)
(zero border), conserved exactly at gamma = 0.  With damping, v' = f (v + h c2s2 lap e), f < 1, one sub-step changes E by
(f - 1) (v~^2 (1 + f) + h w^2 a v~) per mode (v~ the rate before the factor): negative on average over an oscillation but not at every
sub-step, the second term changes sign just behind a turning point (v~ small, a large, of opposite signs).  "The energy never rises at any
sub-step" is therefore false for this update, whatever quadratic energy is taken that the undamped step conserves: the test
test_energy_rises_in_one_substep shows the sub-step (mode (1, 1), gamma = 0.05, sub-step 115: +1.35e-7 E, nine orders above float64 rounding) and that the formula
above predicts it.  The staggered form 1/2 v'^2 + 1/2 w^2 a a' changes by -h gamma v'(v' + v), which has the same defect.  What holds, and
what is asserted: E is conserved to rounding at gamma = 0, and with gamma > 0 E never rises above any value it had a full period of the
slowest mode earlier, and never above where it started.
"""

import numpy as np
import pytest

import ripple64

R = 64


def _mode(p, q):
    i = np.arange(1, R + 1)
    return np.outer(np.sin(np.pi * q * i / (R + 1)), np.sin(np.pi * p * i / (R + 1)))


def _energy(eta, rate, h, c2s2):
    e = np.pad(np.asarray(eta, np.float64), 1)
    g = ((e[1:, :] - e[:-1, :]) ** 2).sum() + ((e[:, 1:] - e[:, :-1]) ** 2).sum()
    lap = (e[1:-1, :-2] + e[1:-1, 2:]) + (e[:-2, 1:-1] + e[2:, 1:-1]) - 4 * e[1:-1, 1:-1]
    return 0.5 * (rate ** 2).sum() + 0.5 * c2s2 * g + 0.5 * h * c2s2 * (rate * lap).sum()


def _run(eta, n, h, c2s2, f, B=0, ox=0, oy=0, mistake=None, src=None):
    rate = np.zeros_like(eta)
    zero = np.zeros((R, R), np.int32)
    out = [(eta, rate)]
    for k in range(n):
        eta, rate = ripple64.substep(eta, rate, src if (k == 0 and src is not None) else zero, ox, oy, B, h, c2s2, f, k == 0, np.float64, mistake)
        out.append((eta, rate))
    return out


@pytest.mark.parametrize("p,q", [(1, 1), (3, 5), (64, 64)])
def test_eigenmode_closed_form(p, q):
    """200 sub-steps of the float64 restatement against the rotation by theta, to 1e-12"""
    s, c, n = 0.5, 2.0, 200
    h, c2s2, f = ripple64.params(c, s, 0.0, 0, 0.0, 0.1, 1)
    h, c2s2 = float(h), float(c2s2)
    lam = (4 / s ** 2) * (np.sin(np.pi * p / (2 * (R + 1))) ** 2 + np.sin(np.pi * q / (2 * (R + 1))) ** 2)
    # (c2s2 is the rounded c^2/s^2: the closed form takes the same number)
    w2 = c2s2 * s ** 2 * lam
    cos = 1 - h * h * w2 / 2
    assert abs(cos) < 1
    theta = np.arccos(cos)
    m = _mode(p, q)
    states = _run(m, n, h, c2s2, f)
    x1 = 1 - h * h * w2                                   # from rest: b' = -h w^2, a' = 1 - h^2 w^2
    for k in (1, 2, 57, n):
        want = np.cos(k * theta) + (x1 - cos) * np.sin(k * theta) / np.sin(theta)
        assert np.abs(states[k][0] - want * m).max() < 1e-12, (k, np.abs(states[k][0] - want * m).max())


def test_energy_conserved_without_damping_and_falls_with_it():
    rng = np.random.default_rng(5)
    eta = rng.normal(size=(R, R))
    h, c2s2, f = ripple64.params(2.0, 0.5, 0.0, 0, 0.0, 0.1, 1)
    E = np.array([_energy(e, v, float(h), float(c2s2)) for e, v in _run(eta, 300, h, c2s2, f)])
    assert np.abs(E / E[0] - 1).max() < 1e-12

    # the slowest mode's period in sub-steps
    lam = (4 / 0.25) * 2 * np.sin(np.pi / (2 * (R + 1))) ** 2
    period = int(np.ceil(2 * np.pi / (float(h) * np.sqrt(4.0 * 0.25 * lam * 4))))
    for gamma, B, sg in [(0.5, 0, 0.0), (0.05, 8, 4.0)]:
        h, c2s2, f = ripple64.params(2.0, 0.5, gamma, B, sg, 0.1, 1)
        E = np.array([_energy(e, v, float(h), float(c2s2)) for e, v in _run(eta, 3 * period, h, c2s2, f, B=B)])
        assert (E[1:] <= E[0]).all()
        assert (E[period:] <= E[:-period]).all()
        assert E[-1] < 0.9 * E[0]


def test_energy_rises_in_one_substep():
    """the concrete sub-step at which the damped step's energy rises, and the per-mode formula that says so (module docstring)"""
    gamma, p, q = 0.05, 1, 1
    h, c2s2, f = ripple64.params(2.0, 0.5, gamma, 0, 0.0, 0.1, 1)
    hh, cc, ff = float(h), float(c2s2), float(f[0])
    m = _mode(p, q)
    states = _run(m, 120, h, c2s2, f)
    E = np.array([_energy(e, v, hh, cc) for e, v in states])
    k = 115
    rise = (E[k + 1] - E[k]) / E[k]
    assert 1e-8 < rise < 1e-6, rise
    assert (np.diff(E)[:k] <= 0).all()                                   # the first rise
    # the mode's amplitudes before that sub-step, and the formula's change of b^2 + w^2 a^2 - h w^2 a b
    w2 = cc * 4 * (np.sin(np.pi * p / (2 * (R + 1))) ** 2 + np.sin(np.pi * q / (2 * (R + 1))) ** 2)
    a, b = states[k][0][0, 0] / m[0, 0], states[k][1][0, 0] / m[0, 0]
    vt = b - hh * w2 * a
    dQ = (ff - 1) * (vt * vt * (1 + ff) + hh * w2 * a * vt)
    assert dQ > 0 and a * vt < 0
    norm = 0.5 * (m * m).sum()
    assert abs(dQ * norm - (E[k + 1] - E[k])) <= 1e-6 * abs(E[k + 1] - E[k])


def _reference_case(mistake=None):
    """a random state with deposits pending on the border and inside, the sponge on, the window wrapping the torus: four sub-steps"""
    rng = np.random.default_rng(11)
    lay = ripple64.Layer(R, 0.5, np.float64, B=8)
    lay.move(37, -21)
    lay.set_window(rng.normal(size=(R, R)), rng.normal(size=(R, R)), rng.integers(-2 ** 20, 2 ** 20, (R, R)))
    lay.step(0.2, 4, mistake)
    return lay.window()


@pytest.mark.parametrize("mistake", ripple64.MISTAKES)
def test_planted_mistakes_fail(mistake):
    good, bad = _reference_case(), _reference_case(mistake)
    assert np.abs(good - bad).max() > 1e-3 * np.abs(good).max(), mistake


def test_explicit_order_breaks_the_closed_form():
    """the explicit order (height with the OLD rate) grows: it is not the rotation"""
    h, c2s2, f = ripple64.params(2.0, 0.5, 0.0, 0, 0.0, 0.1, 1)
    m = _mode(3, 5)
    good = _run(m, 200, h, c2s2, f)[-1][0]
    bad = _run(m, 200, h, c2s2, f, mistake="explicit")[-1][0]
    assert np.abs(good).max() <= 1 + 1e-9 and np.abs(good - bad).max() > 1e-2


def test_sponge_index_and_table():
    wx, wy = ripple64.window_coords(R, 0, 0)
    k = ripple64.sponge_index(wx, wy, R, 8)
    assert k[0, 0] == 8 and k[0, 30] == 8 and k[1, 30] == 7 and k[7, 30] == 1 and k[8, 30] == 0 and k[30, R - 1] == 8 and k[30, R - 8] == 1
    assert ripple64.sponge_index(wx, wy, R, 0).max() == 0
    h, _, f = ripple64.params(2.0, 0.5, 0.05, 8, 4.0, 0.1, 2)
    assert len(f) == 9 and f.dtype == np.float32 and (np.diff(f) < 0).all()
    assert f[0] == np.float32(1 / (1 + float(h) * 0.05000000074505806)) and f[8] == np.float32(1 / (1 + float(h) * (0.05000000074505806 + 4.0)))


def test_stability_bound():
    assert ripple64.stable(2.0, 0.5, 0.1, 1) and not ripple64.stable(2.0, 0.5, 0.2, 1) and ripple64.stable(2.0, 0.5, 0.2, 2)
    assert ripple64.stable(2.0, 0.5, 0.0, 1) and not ripple64.stable(2.0, 0.5, -0.01, 1)
