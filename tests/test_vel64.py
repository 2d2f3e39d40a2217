"""CPU tests of the surface velocity's references (tests/vel64.py): the float64 definition against the central difference of
displace64, single bins in closed form, the planted mistakes, and the constant of the GPU tests' bar."""

import numpy as np
import pytest

import pointwise as pw
import ref64
import vel64

F = np.float32


def _state(oracle, N, steps=3):
    p = oracle.EXAMPLE
    ws, chop = p["wavescale"], p["choppiness"]
    h0 = pw.lit_state(oracle, N)
    phase = pw.lit_phase(oracle, N, ws, steps)
    return h0, phase, ws, chop, F(1) / F(ws), vel64.omega32(N, ws)


def _central(h0, phase, omega, scale, chop, delta):
    """(displace64(phase + omega delta) - displace64(phase - omega delta)) / (2 delta), the three displacement channels, float64 phases"""
    ph = phase.astype(np.float64)
    om = omega.astype(np.float64)
    hi = ref64.displace64(h0, ph + om * delta, scale, chop)[:3]
    lo = ref64.displace64(h0, ph - om * delta, scale, chop)[:3]
    return (hi - lo) / (2 * delta)


def test_vel64_is_the_limit_of_the_central_difference(oracle):
    N = 64
    h0, phase, ws, chop, scale, om = _state(oracle, N)
    v = vel64.vel64(h0, phase, scale, chop, om)
    # omega delta << 1 for the largest omega (about 9.4 rad/s at this scale): the error is the cubic term, a quarter per halving
    deltas = (4e-3, 2e-3, 1e-3)
    errs = [float(np.abs(_central(h0, phase, om, scale, chop, d) - v).max()) for d in deltas]
    ratios = [errs[i] / errs[i + 1] for i in range(2)]
    print(f"central difference against vel64: errors {errs}, ratios {ratios}")
    assert all(3.5 <= r <= 4.5 for r in ratios), (errs, ratios)


@pytest.mark.parametrize("bin_", [(0, 0), (63, 63), (32, 33), (0, 32), (20, 45)])
def test_single_bin_closed_form(bin_):
    # vel64 texel by texel against the two plane waves written out (vel64.single_bin64): each has the amplitude omega |a| of ITS texel and
    # runs a quarter period ahead of its displacement
    N, ws, chop = 64, 22.0, 1.3
    scale = F(1) / F(ws)
    om = vel64.omega32(N, ws)
    a = (F(0.3), F(-0.2))
    h0 = np.zeros((N, N, 2), np.float32)
    h0[bin_] = a
    rs = np.random.RandomState(5)
    phase = (rs.random_sample((N, N)) * 6.28).astype(np.float32)
    v = vel64.vel64(h0, phase, scale, chop, om)
    want = vel64.single_bin64(N, bin_, a, phase, scale, chop, om)
    mirror = (N - 1 - bin_[0], N - 1 - bin_[1])
    amp = (float(om[bin_]) + float(om[mirror])) * float(np.hypot(a[0], a[1]))
    assert np.abs(v - want).max() <= 1e-11 * amp
    # a single wave (the mirror's omega set to 0) has amplitude exactly omega |a| up to the grid's sampling of the crest
    ob = om.astype(np.float64).copy()
    ob[mirror] = 0
    w1 = vel64.single_bin64(N, bin_, a, phase, scale, chop, ob)[2]
    assert np.abs(w1).max() <= float(om[bin_]) * float(np.hypot(a[0], a[1])) * (1 + 1e-12)
    # ... and stands a quarter period ahead of the displacement: omega_b dz(phase + pi / 2) with the mirror texel's wave taken out
    hb = np.zeros((N, N), np.complex128)
    hb[bin_] = complex(a[0], a[1]) * np.exp(1j * (float(phase[bin_]) + np.pi / 2))
    ahead = ref64.transform2(hb).real * ref64._sign(N)
    assert np.abs(w1 - float(om[bin_]) * ahead).max() <= 1e-11 * amp


def test_k_zero_gives_exactly_zero():
    # omega(k = 0) = 0: the texel of the spectrum at k = 0 is exactly zero whatever h0 and the phase hold there, in fp32 and in float64.
    # (The bin's h0 also enters ocean.sim's mirror texel (N/2 - 1, N/2 - 1), which has a k of its own and moves; with that texel's omega
    # taken out nothing is left.)
    N, ws = 64, 22.0
    h = N // 2
    h0 = np.zeros((N, N, 2), np.float32)
    h0[h, h] = (0.3, -0.2)
    phase = np.full((N, N), 0.7, np.float32)
    om = vel64.omega32(N, ws)
    assert om[h, h] == 0 and om[h - 1, h - 1] > 0
    knx, kny = vel64.khat32(N, F(1) / F(ws))
    assert knx[h, h] == 0 and kny[h, h] == 0
    for f in vel64.spectrum32(h0, np.sin(phase), np.cos(phase), om, knx, kny):
        assert np.all(f[h, h] == 0)
    om[h - 1, h - 1] = 0
    assert np.all(vel64.vel64(h0, phase, F(1) / F(ws), 1.3, om) == 0)


@pytest.mark.parametrize("mistake", ["mirror", "omega", "chop"])
def test_planted_mistakes_fail(oracle, mistake):
    N = 64
    h0, phase, ws, chop, scale, om = _state(oracle, N)
    # (an asymmetric table for "omega": the true one is symmetric under the mirror but for its first row and column)
    ref = vel64.vel64(h0, phase, scale, chop, om)
    bad = vel64.vel64(h0, phase, scale, chop, om, mistake=mistake)
    k = vel64.k_of(bad, ref, N)
    print(f"planted mistake {mistake}: K {k:.3g} (bar {vel64.K_VEL:.3g})")
    assert k > vel64.K_VEL


def test_the_restatement_sets_the_bar(oracle):
    worst = 0.0
    for N in vel64.VEL_SIZES:
        h0, phase, ws, chop, scale, om = _state(oracle, N, vel64.VEL_STEPS)
        ref = vel64.vel64(h0, phase, scale, chop, om)
        got = vel64.vel32(oracle, h0, phase, om, scale, chop).astype(np.float64)
        k = vel64.k_of(got, ref, N)
        print(f"vel32 against vel64, N = {N}: K {k:.3f}")
        worst = max(worst, k)
    assert worst <= vel64.K_REF_VEL <= 1.05 * worst, worst
    assert vel64.K_VEL == 3 * vel64.K_REF_VEL


def test_fma32_rounds_once():
    rs = np.random.RandomState(3)
    a, b = rs.standard_normal(4096).astype(np.float32), rs.standard_normal(4096).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)        # cancellation: the product's low bits decide
    got = vel64.fma32(a, b, c)
    from fractions import Fraction
    for i in range(0, 4096, 64):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert float(got[i]) == float(np.float32(float(exact))) or abs(exact) < Fraction(1, 2 ** 140), i
