"""Body stepping's arithmetic (datum_amd/csrc/ocean_step.h), the very functions ocean_step_kernel calls, walked on the CPU
(tests/cpu/step_emul.cpp) on random velocity records, poses, motions, props and ranges:

  * the ten sums of a sub-step against body64.reduce32 (fields 0-2) and drag64.reduce32 (fields 0-5, 7) on the same records: bit for bit,
    for the counts 0, 1, 63, 64, 65, 129 and 1000;
  * step_integrate against step64.integrate32, the definition of include/datum_ocean_hip.h in numpy float32: bit for bit, poses, motions,
    force and torque, and step_state_finite against its rule;
  * integrate32 against integrate64, the same formulas in float64 from the same fp32 inputs.  With eps = 2^-24 and g(n) = n eps / (1 - n eps):
    a value that a chain of n roundings separates from its inputs lies within g(n) A of the float64 value, A the same expression with
    every term replaced by its magnitude.  The depths n (roundings on the longest path, counted in the header's formulas):
        force 2, torque 2, v' 6, T' 8, tau_b 5, alpha_b 6, alpha 9, omega' 11, c_j' 15
    The rotation is not a polynomial; to first order (the second-order terms are below 1e-5 of these here, covered by the factor
    SECOND = 1 + 1e-3), with dc_j the bar of c_j' as a vector (its Euclidean norm), n0 = |c_0'|, n1 = |y0|:
        dx  = dc_0 / n0 + 5 eps                         the norm's four roundings and the division, |x_k| <= 1
        dy0 = dc_1 + 2 sqrt(3) |c_1'| dx + 5 eps |c_1'|     c_1' itself; x twice in (x.c) x; the dot's three roundings, product, difference
        dy  = dy0 / n1 + 5 eps
        dz  = 2 (dx + dy) + 3 eps                       z = x X y: two products and a difference of values below 1
"""

import ctypes
import os

import numpy as np
import pytest

import body64
import drag64
import step64
from test_body_emul import _case
from test_drag_emul import COUNTS, _motions, _records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
EPS = 2.0 ** -24
SECOND = 1.0 + 1e-3


def g(n):
    return n * EPS / (1 - n * EPS)


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpu", "libfft_core_emul.so"))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.step_reduce.argtypes = [P, P, P, I, P, I, P, P, P, P]
    lib.step_integrate_bodies.argtypes = [P, P, P, I, P, ctypes.c_float, P, P]
    return lib


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _props(rng, nb):
    b = np.arange(nb)
    p = step64.make_props(1.0 / rng.uniform(200, 5000, nb), 1.0 / rng.uniform(100, 5000, (nb, 3)), 9.81, 9810.0)
    p["invmass"][b % 6 == 2] = 0
    p["invinertia"][b % 7 == 4, 1] = 0
    return p


def _reduce(emul, bodies, motions, props, probes, recs):
    off, rows = body64.offsets(bodies, len(probes))
    assert len(recs) == rows
    bodies, motions, props = np.ascontiguousarray(bodies), np.ascontiguousarray(motions), np.ascontiguousarray(props)
    probes, recs = np.ascontiguousarray(probes, F), np.ascontiguousarray(recs, F)
    sums, bad = np.full((len(bodies), 10), -7.0, F), np.full(len(bodies), -1, np.int32)
    emul.step_reduce(bodies.ctypes.data, motions.ctypes.data, props.ctypes.data, len(bodies), probes.ctypes.data, len(probes), off.ctypes.data, recs.ctypes.data,
                     sums.ctypes.data, bad.ctypes.data)
    return sums, bad.astype(bool)


def _integrate(emul, bodies, motions, props, sums, h):
    b, m = np.ascontiguousarray(bodies).copy(), np.ascontiguousarray(motions).copy()
    sums = np.ascontiguousarray(sums, F)
    totals, finite = np.zeros((len(b), 6), F), np.zeros(len(b), np.int32)
    emul.step_integrate_bodies(b.ctypes.data, m.ctypes.data, np.ascontiguousarray(props).ctypes.data, len(b), sums.ctypes.data, F(h), totals.ctypes.data, finite.ctypes.data)
    return b, m, totals, finite.astype(bool)


def _setup(seed, counts):
    rng = np.random.RandomState(seed)
    bodies, probes = _case(rng, counts)
    motions, props = _motions(rng, len(counts)), _props(rng, len(counts))
    recs = _records(rng, body64.offsets(bodies, len(probes))[1], extremes=False)
    return bodies, motions, props, probes, recs


def test_sums_are_the_two_calls_fields_bit_for_bit(emul):
    bodies, motions, props, probes, recs = _setup(31, COUNTS * 6)
    sums, bad = _reduce(emul, bodies, motions, props, probes, recs)
    lift, drag = body64.reduce32(bodies, probes, recs), drag64.reduce32(bodies, motions, probes, recs)
    assert not bad.any() and np.isfinite(sums).all()
    assert np.array_equal(_bits(sums), _bits(step64.sums32(lift, drag)))
    assert np.all(sums[0] == 0) and not np.signbit(sums[0]).any()            # count == 0: ten +0.0
    assert np.abs(sums[:, :9]).min(0).max() >= 0 and (np.abs(sums[:, 1:9]).max(0) > 1).all()

    # the rules that make a body bad before its walk, and a bad probe
    b2, m2, p2, pr2 = bodies.copy(), motions.copy(), props.copy(), probes.copy()
    b2["cap"][8] = np.nan
    m2["angular"][9, 1] = np.inf
    p2["invmass"][10], p2["invinertia"][11, 2], p2["gravity"][12], p2["buoyancy"][13] = np.nan, np.inf, -np.inf, np.nan
    p2["pad"][15] = np.nan                                                     # the padding is not looked at
    off1, rows1 = body64.offsets(b2, len(probes))
    off0, _ = body64.offsets(bodies, len(probes))
    recs1 = np.zeros((rows1, 8), F)
    for b in range(len(bodies)):
        if not body64.range_bad(b2, len(probes))[b]:
            recs1[off1[b]:off1[b] + bodies["count"][b]] = recs[off0[b]:off0[b] + bodies["count"][b]]
    _, bad = _reduce(emul, b2, m2, p2, pr2, recs1)
    assert bad.nonzero()[0].tolist() == [8, 9, 10, 11, 12, 13]
    assert step64.props_bad(p2).nonzero()[0].tolist() == [10, 11, 12, 13]


def test_integrate_matches_integrate32_bit_for_bit(emul):
    bodies, motions, props, probes, recs = _setup(32, COUNTS * 6)
    lift, drag = body64.reduce32(bodies, probes, recs), drag64.reduce32(bodies, motions, probes, recs)
    sums = step64.sums32(lift, drag)
    for dt, sub in ((1 / 60, 1), (1 / 60, 3), (0.25, 16), (-1 / 30, 2)):
        h = step64.step_size(dt, sub)
        gb, gm, totals, finite = _integrate(emul, bodies, motions, props, sums, h)
        wb, wm, wr, bad = step64.integrate32(lift, drag, bodies, motions, props, h)
        assert finite.all() and not bad.any()
        assert np.array_equal(_bytes(gb), _bytes(wb)), (dt, sub)
        assert np.array_equal(_bytes(gm), _bytes(wm)), (dt, sub)
        assert np.array_equal(_bits(totals), _bits(wr[:, :6])), (dt, sub)
        assert (gb["rotation"] != bodies["rotation"]).any() and (gb["position"] != bodies["position"]).any()
    # two sub-steps in a row: the second starts from the first's pose
    h = step64.step_size(1 / 60, 2)
    b1, m1, _, _ = _integrate(emul, bodies, motions, props, sums, h)
    b2, m2, _, _ = _integrate(emul, b1, m1, props, sums, h)
    w1 = step64.integrate32(lift, drag, bodies, motions, props, h)
    w2 = step64.integrate32(lift, drag, w1[0], w1[1], props, h)
    assert np.array_equal(_bytes(b2), _bytes(w2[0])) and np.array_equal(_bytes(m2), _bytes(w2[1]))

    # a column of length zero, an overflowing velocity: not finite, and integrate32 keeps the body as it was
    zb, zm, big = bodies.copy(), motions.copy(), sums.copy()
    zb["rotation"][5].reshape(3, 3)[:, 0] = 0
    zm["angular"][5] = 0
    zp = props.copy()
    zp["invinertia"][5] = 0
    big[6, 5] = 3e38
    zp["invmass"][6] = 1.0
    _, _, _, finite = _integrate(emul, zb, zm, zp, big, F(10.0))
    assert finite.nonzero()[0].tolist() == [b for b in range(len(bodies)) if b not in (5, 6)]
    dr = drag.copy()
    dr[6, 2] = 3e38
    wb, wm, wr, bad = step64.integrate32(lift, dr, zb, zm, zp, F(10.0))
    assert bad.nonzero()[0].tolist() == [5, 6] and np.isnan(wr[[5, 6]]).all()
    assert np.array_equal(_bytes(wb[[5, 6]]), _bytes(zb[[5, 6]])) and np.array_equal(_bytes(wm[[5, 6]]), _bytes(zm[[5, 6]]))


def test_integrate32_lies_within_counted_roundings_of_integrate64(report):
    bodies, motions, props, probes, recs = _setup(33, [1, 2, 63, 64, 65, 129, 200, 1000] * 5)
    lift, drag = body64.reduce32(bodies, probes, recs), drag64.reduce32(bodies, motions, probes, recs)
    worst = {}
    for dt, sub in ((1 / 60, 1), (1 / 60, 4), (0.1, 1)):
        h = step64.step_size(dt, sub)
        gb, gm, gr, bad = step64.integrate32(lift, drag, bodies, motions, props, h)
        assert not bad.any()
        w = step64.integrate64(lift, drag, bodies, motions, props, h)
        D = np.float64
        ah = abs(D(h))
        R, T = np.abs(bodies["rotation"].astype(D)), np.abs(bodies["position"].astype(D))
        v, o = np.abs(motions["linear"].astype(D)), np.abs(motions["angular"].astype(D))
        im, ii, gr_, rho = (np.abs(props[k].astype(D)) for k in ("invmass", "invinertia", "gravity", "buoyancy"))
        L, Dg = np.abs(lift.astype(D)), np.abs(drag.astype(D))
        AF = np.stack([Dg[:, 0], Dg[:, 1], rho * L[:, 0] + Dg[:, 2]], 1)
        AQ = np.stack([rho * L[:, 1] + Dg[:, 3], rho * L[:, 2] + Dg[:, 4], Dg[:, 5]], 1)
        Av = v + ah * (AF * im[:, None] + np.stack([0 * gr_, 0 * gr_, gr_], 1))
        AT = T + ah * Av
        R3 = R.reshape(-1, 3, 3)
        Ab = np.einsum("nij,ni->nj", R3, AQ) * ii                          # tau_b, alpha_b: R transposed
        Aa = np.einsum("nkj,nj->nk", R3, Ab)
        Ao = o + ah * Aa
        bars = dict(force=g(2) * AF, torque=g(2) * AQ, linear=g(6) * Av, position=g(8) * AT, angular=g(11) * Ao)
        got = dict(force=gr[:, :3], torque=gr[:, 3:6], linear=gm["linear"], position=gb["position"], angular=gm["angular"])

        def cross_abs(a, c):
            return np.stack([a[:, 1] * c[:, 2] + a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] + a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] + a[:, 1] * c[:, 0]], 1)

        dc, cn = [], []
        for j in range(2):
            col = R3[:, :, j]
            dc.append(np.sqrt(((g(15) * (col + ah * cross_abs(Ao, col))) ** 2).sum(1)))
            # c_j' itself, in float64
            c0 = bodies["rotation"].astype(D).reshape(-1, 3, 3)[:, :, j]
            cn.append(c0 + D(h) * np.cross(w["angular"], c0))
        n0 = np.linalg.norm(cn[0], axis=1)
        x = cn[0] / n0[:, None]
        y0 = cn[1] - (x * cn[1]).sum(1)[:, None] * x
        n1 = np.linalg.norm(y0, axis=1)
        c1 = np.linalg.norm(cn[1], axis=1)
        dx = dc[0] / n0 + 5 * EPS
        dy0 = dc[1] + 2 * np.sqrt(3.0) * c1 * dx + 5 * EPS * c1
        dy = dy0 / n1 + 5 * EPS
        dz = 2 * (dx + dy) + 3 * EPS
        bars["rotation"] = SECOND * np.stack([dx, dy, dz] * 3, 1)
        got["rotation"] = gb["rotation"]
        for name, bar in bars.items():
            err = np.abs(got[name].astype(D) - w[name])
            ok = bar > 0
            assert np.all(err[~ok] == 0), name
            ratio = float((err[ok] / bar[ok]).max())
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert ratio <= 1.0, (name, dt, sub, ratio)
    report("step: integrate32 against integrate64, worst |error| / bar: " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()))
