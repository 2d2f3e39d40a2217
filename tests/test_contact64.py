"""Closed forms on the float64 model of body contact (tests/contact64.py: Land64 -- gravity and contact alone, no water), and the planted
mistakes, each of which must show.

The box: 5 x 5 probes of weight a = 0.04 m^2 on a 1 m square (sum a = 1 m^2), 100 kg, on flat land 0.5 m above the sea (raw = -0.5
everywhere).  k = 2.0e4 N/m per m^2: p* = gravity / (k sum a invmass) = 9.81 / 200 = 0.04905 m, and the bound h sqrt(k sum a invmass) < 2
gives h < 0.1414 s."""

import numpy as np
import pytest

import body64
import contact64
import drag64
import step64

K, MASS, G = 2.0e4, 100.0, 9.81
LAND = 0.5
# the model takes poses, props and maps as the float32 arrays the call takes: every input carries up to 2^-24 of itself (6e-8 at 1, 6e-7
# at 9.81), and the closed forms below combine a handful of them: 1e-6 of the quantity's scale bounds that, and no mistake hides in it
TOL = 1.0e-6


def _box(z, v=(0.0, 0.0, 0.0), rot=None):
    g = np.linspace(-0.5, 0.5, 5)
    x, y = np.meshgrid(g, g)
    probes = np.stack([x.ravel(), y.ravel(), np.zeros(25), np.full(25, 0.04)], 1).astype(np.float32)
    bodies = body64.make_bodies([np.eye(3) if rot is None else rot], [[0.0, 0.0, z]], [0], [25], [np.inf])
    motions = drag64.make_motions([v], [[0.0, 0.0, 0.0]], [0.0], [0.0])
    props = step64.make_props([1.0 / MASS], [[0.0, 0.0, 0.0]], G, 0.0)                 # no buoyancy, no spin-up
    return bodies, motions, props, probes


def _flat(c=0.0, ct=0.0, slope=0.0, k=K):
    """land LAND above the sea, rising by `slope` per metre of x (the depth falls)"""
    W = 9
    x = (np.arange(W) - 4) * 5.0
    depths = np.repeat((-LAND - slope * x)[None, :], W, 0)
    return contact64.make_scene(k, c, ct, contact64.BED, dict(origin=(-20.0, -20.0), texel=5.0, outside=50.0), depths)


def _energy(m, p):
    """kinetic + gravitational + the spring's, per the model: p the penetration of the flat box"""
    v = m.v[0]
    return 0.5 * MASS * float(v @ v) + MASS * G * float(m.T[0, 2]) + 0.5 * K * max(p, 0.0) ** 2


def test_box_rests_at_the_closed_form_penetration():
    pstar = G / (K * 1.0 / MASS)
    m = contact64.Land64(*_box(LAND - pstar), _flat(c=0.0))
    for _ in range(200):
        m.substep(0.005)
    assert abs(LAND - m.T[0, 2] - pstar) < TOL and abs(m.v[0, 2]) < TOL and m.count[0] == 25
    assert abs(m.deepest[0] - pstar) < TOL and abs(m.force[0, 2] - MASS * G) < TOL * MASS * G
    # dropped with damping, it settles there
    m = contact64.Land64(*_box(LAND + 0.2), _flat(c=2.0e3))
    for _ in range(4000):
        m.substep(0.005)
    assert abs(LAND - m.T[0, 2] - pstar) < 1e-6 and abs(m.v[0, 2]) < 1e-6


def test_energy_never_rises_with_damping_and_stays_bounded_without():
    h = 0.01                                                                           # h sqrt(k sum a / m) = 0.141
    m = contact64.Land64(*_box(LAND + 0.3), _flat(c=1.0e3))
    # (semi-implicit Euler conserves a shadow energy that differs from E by O(h): the envelope is held, with that margin)
    e0 = _energy(m, 0.0)
    margin = 0.5 * h * np.sqrt(K / MASS) * e0
    peak = []
    last = e0
    for i in range(3000):
        m.substep(h)
        e = _energy(m, LAND - m.T[0, 2])
        assert e <= last + margin
        if i % 500 == 499:
            peak.append(e)
            last = min(last, e)
    # (at rest the samples repeat to the last bit or two of the float64 sum that forms them)
    assert all(b <= a * (1 + 1e-12) for a, b in zip(peak, peak[1:])) and peak[-1] < e0 - 0.9 * MASS * G * 0.3
    # no damping, inside the bound: bounded for ever (the bounce returns to its drop height, within the shadow energy's O(h))
    m = contact64.Land64(*_box(LAND + 0.3), _flat(c=0.0))
    top = []
    for i in range(20000):
        m.substep(h)
        top.append(m.T[0, 2])
    top = np.array(top)
    assert top.max() < LAND + 0.3 * 1.2 and top[-5000:].max() > LAND + 0.3 * 0.8 and np.isfinite(top).all()
    # outside the bound it is not: the documented bound is the real one
    m = contact64.Land64(*_box(LAND - 0.01), _flat(c=0.0))
    for i in range(400):
        m.substep(0.2)
    assert not abs(m.T[0, 2]) < 10.0


def test_sliding_slows_at_the_rate_friction_gives():
    """on flat land at rest depth the tangential force is -sum a ct v: v(t) = v0 (1 - h sum a ct / m)^n under semi-implicit Euler"""
    ct, h, n, pstar = 300.0, 0.005, 400, G / (K / MASS)
    m = contact64.Land64(*_box(LAND - pstar, v=(2.0, -1.0, 0.0)), _flat(c=0.0, ct=ct))
    for _ in range(n):
        m.substep(h)
    want = np.array([2.0, -1.0]) * (1.0 - h * ct / MASS) ** n
    assert np.allclose(m.v[0, :2], want, rtol=TOL, atol=0) and abs(m.v[0, 2]) < TOL
    # on a slope the normal is tilted by it: the box slides downhill (towards -x, where the land is lower)
    m = contact64.Land64(*_box(LAND - pstar), _flat(c=2.0e3, ct=0.0, slope=0.1))
    for _ in range(400):
        m.substep(h)
    assert m.v[0, 0] < -0.1 and abs(m.v[0, 1]) < 1e-12


def test_hull_comes_back_from_a_box_wall_no_faster_than_it_came():
    walls = contact64.make_walls([(5.0, 0.0, 1.0, 0.0, 2.0, 50.0, contact64.BOX)])          # its face at x = 3
    for c in (0.0, 500.0):
        scene = contact64.make_scene(K, c, 0.0, contact64.WALLS, walls=walls)
        b, mo, pr, probes = _box(0.0, v=(1.5, 0.0, 0.0))
        pr["gravity"] = 0.0
        m = contact64.Land64(b, mo, pr, probes, scene)
        deepest = 0.0
        for _ in range(4000):
            m.substep(0.002)
            deepest = max(deepest, float(m.deepest[0]))
        assert m.v[0, 0] < 0 and abs(m.v[0, 0]) <= 1.5 * (1 + 1e-3) and m.T[0, 0] < 2.5 and deepest > 0.01
        if c > 0:
            assert abs(m.v[0, 0]) < 1.4


@pytest.mark.parametrize("mistake", contact64.MISTAKES)
def test_planted_mistakes_show(mistake):
    h, pstar = 0.005, G / (K / MASS)
    if mistake == "normal_sign":
        m = contact64.Land64(*_box(LAND - pstar), _flat(), mistake=mistake)
        for _ in range(100):
            m.substep(h)
        assert m.T[0, 2] < LAND - 10 * pstar                                           # the ground pulls it in
    elif mistake == "no_clamp":
        # leaving the ground fast with heavy damping: the unclamped force is negative, the ground holds the hull back
        good, wrong = (contact64.Land64(*_box(LAND - 0.01, v=(0, 0, 3.0)), _flat(c=5.0e4), mistake=x) for x in (None, mistake))
        good.substep(h), wrong.substep(h)
        assert good.force[0, 2] == 0.0 and wrong.force[0, 2] < -1000.0
    elif mistake == "no_inv2":
        walls = contact64.make_walls([(5.0, 0.0, 2.0, 0.0, 4.0, 100.0, contact64.BOX)])      # an axis of length 2: its face at x = 3
        scene = contact64.make_scene(K, 0.0, 0.0, contact64.WALLS, walls=walls)
        b, mo, pr, probes = _box(0.0)
        b["position"][0, 0] = 3.0                                                      # half the probes 0 .. 0.5 m inside
        good, wrong = (contact64.Land64(b, mo, pr, probes, scene, mistake=x) for x in (None, mistake))
        good.substep(h), wrong.substep(h)
        # |n| = 2 and p = q / 4: the spring force is k a (world depth); without inv2 it is four times that
        depth = np.array([0.25, 0.5] * 5)
        assert abs(good.force[0, 0] + K * 0.04 * depth.sum()) < TOL * 3000 and abs(wrong.force[0, 0] / good.force[0, 0] - 4.0) < TOL
        assert abs(good.deepest[0] - 0.25) < TOL                                     # q / 4 with q = 2 * 0.5: the documented p
    elif mistake == "origin_arm":
        b, mo, pr, probes = _box(LAND - pstar)
        b["position"][0, :2] = (7.0, -3.0)
        good, wrong = (contact64.Land64(b, mo, pr, probes, _flat(), mistake=x) for x in (None, mistake))
        kg, kw = good.contact(), wrong.contact()
        assert np.abs(kg[0, 3:6]).max() < TOL * MASS * G and np.abs(kw[0, 3:6]).max() > 100.0        # a level box on flat land feels no torque
    else:
        good, wrong = (contact64.Land64(*_box(LAND - pstar), _flat(), mistake=x) for x in (None, mistake))
        assert abs(good.contact()[0, 7] - pstar) < TOL and abs(wrong.contact()[0, 7] - 25 * pstar) < TOL
